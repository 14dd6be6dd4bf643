"""NumPy oracle of the Eagle step kernels (eagle_step.hip, float and double).

splitmix64 on np.uint64 with the constants of csrc/common.h, the 24-bit
uniform, Laplace and Gumbel, and the suggest / update formulas of
vizier_amd/_src/algorithms/optimizers/eagle.py as the kernels evaluate
them, for q >= 1. Shared by tests/test_fp64_kernels.py and
tests/test_eagle_kernels.py (GPU) and tests/test_fp64_dispatch.py (CPU:
hard-coded splitmix64 / uniform values).

`dtype` is the kernel's number format: inputs, config constants and RNG
draws are rounded to it, because that is what the kernel is handed.
np.float64 (the default) is the fp64 kernels' oracle; np.float32
reproduces vz_rng_uniform bit for bit. `arith` (suggest only) is the
format the formulas are evaluated in: float64 for the reference,
float32 to measure how far plain float32 evaluation moves the result.
`update` has one multiply and compares only, so it evaluates in `dtype`
and is compared bitwise.
"""

import dataclasses
import math

import numpy as np

_U64 = np.uint64
_GOLDEN = _U64(0x9e3779b97f4a7c15)
_MUL1 = _U64(0xbf58476d1ce4e5b9)
_MUL2 = _U64(0x94d049bb133111eb)

# XOR tags the kernels put on the iteration offset per random stream.
TAG_CAT_NOISE = 0x9e01
TAG_GUMBEL = 0x77aa
TAG_REFILL_CONT = 0x5151
TAG_REFILL_CAT = 0x1234
UPDATE_SEED_XOR = 0xABCDEF


def splitmix64(z) -> np.ndarray:
  """vz_splitmix64 of common.h, elementwise on uint64 (wrapping)."""
  z = np.asarray(z, dtype=_U64)
  with np.errstate(over='ignore'):
    z = z + _GOLDEN
    z = (z ^ (z >> _U64(30))) * _MUL1
    z = (z ^ (z >> _U64(27))) * _MUL2
    return z ^ (z >> _U64(31))


def uniform(seed: int, offset: int, idx, dtype=np.float64) -> np.ndarray:
  """((h >> 40) + 0.5) / 2^24 with h = mix(seed ^ mix(offset ^ idx)).

  float32 evaluates it as vz_rng_uniform does, `(float(k) + 0.5f) * 2^-24f`:
  the sum rounds to even once k >= 2^23, and k = 2^24 - 1 gives exactly 1.
  """
  idx = np.asarray(idx, dtype=np.uint32).astype(_U64)
  h = splitmix64(_U64(seed) ^ splitmix64(_U64(offset) ^ idx))
  k = h >> _U64(40)
  if dtype == np.float32:
    return (k.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
  return (k.astype(np.float64) + 0.5) / 16777216.0


def laplace(seed: int, offset: int, idx, dtype=np.float64,
            arith=np.float64) -> np.ndarray:
  """vz_rng_laplace: the uniform in `dtype`, log1p in `arith`."""
  u = uniform(seed, offset, idx, dtype).astype(arith) - arith(0.5)
  a = np.minimum(np.abs(u), arith(dtype(0.499999)))
  return np.where(u >= 0.0, arith(-1.0), arith(1.0)) * np.log1p(
      arith(-2.0) * a)


@dataclasses.dataclass
class Config:
  """EagleStrategyConfig fields the kernels take."""
  visibility: float = 0.45
  gravity: float = 1.5
  negative_gravity: float = 0.008
  normalization_scale: float = 0.5
  cat_factor: float = 1.0
  p_same: float = 0.98
  penalize_factor: float = 0.7
  perturbation_lower_bound: float = 7e-5
  perturbation: float = 0.16


def steady_pool(pool, q, dc, cat_sizes, seed):
  """Test input shared by the kernel tests: a steady-state pool (P, q, Dc)
  / (P, q, Dcat) with a few -inf rewards and spread perturbations, in
  float64 (the float32 tests round it)."""
  rng = np.random.default_rng(seed)
  pool_cont = rng.random((pool, q, dc))
  pool_cat = np.stack([rng.integers(0, s, size=(pool, q))
                       for s in cat_sizes], axis=-1).astype(np.int64) \
      if cat_sizes else np.zeros((pool, q, 0), dtype=np.int64)
  rewards = rng.normal(size=pool)
  rewards[rng.choice(pool, 3, replace=False)] = -np.inf
  perts = 0.16 * 0.7 ** rng.integers(0, 6, size=pool)
  return pool_cont, pool_cat, rewards, perts


def _log(x, arith):
  """log of a scalar already held in `arith`, rounded to `arith`."""
  return arith(math.log(float(x)))


def suggest(pool_cont, pool_cat, rewards, perts, cat_sizes, offset: int,
            n_batches: int, batch_size: int, seed: int, cfg: Config,
            dtype=np.float64, arith=np.float64, return_vals: bool = False):
  """pool_cont (P, q, Dc) float, pool_cat (P, q, Dcat) int64, q >= 1.

  Returns (out_cont (B, q, Dc), out_cat (B, q, Dcat), margin): margin is
  the smallest gap between the best and second-best `logit + gumbel` over
  every categorical entry (inf without categoricals). With `return_vals`
  a fourth value holds every `logit + gumbel`, (B, q * Dcat, max_cat),
  NaN past a dimension's size.

  Distances run over the flat q * Dc / q * Dcat features with n_features =
  Dc + Dcat, the continuous noise is divided by its max-abs over the q
  axis (q = 1: its sign), and the categorical draws are indexed
  b * q * Dcat + jd, as in eagle_suggest_kernel.
  """
  w = arith
  pool_size, q, dc = pool_cont.shape
  dcat = pool_cat.shape[2]
  n_features = dc + dcat
  flat_c, flat_k = q * dc, q * dcat
  max_cat = int(max(cat_sizes)) if dcat else 0
  flat = pool_cont.astype(dtype).astype(w).reshape(pool_size, flat_c)
  cats = pool_cat.reshape(pool_size, flat_k)
  rewards = rewards.astype(dtype).astype(w)
  perts = perts.astype(dtype).astype(w)
  visibility, gravity, neg_gravity, norm_scale, cat_factor, p_same = (
      w(dtype(v)) for v in (cfg.visibility, cfg.gravity,
                            cfg.negative_gravity, cfg.normalization_scale,
                            cfg.cat_factor, cfg.p_same))
  start = (offset % n_batches) * batch_size
  out_cont = np.empty((batch_size, q, dc), dtype=w)
  out_cat = np.empty((batch_size, q, dcat), dtype=np.int64)
  all_vals = np.full((batch_size, flat_k, max_cat), np.nan)
  margin = math.inf
  for b in range(batch_size):
    me = start + b
    diff = flat[me][None, :] - flat
    d2 = (diff * diff).sum(-1) + (cats != cats[me][None, :]).sum(-1).astype(w)
    with np.errstate(invalid='ignore'):   # -inf - -inf: s is zeroed below
      direction = np.where(rewards - rewards[me] >= 0.0, gravity,
                           -neg_gravity)
    force = np.exp(-visibility * d2 / w(n_features) * w(10.0))
    s = np.where(np.isfinite(rewards), direction * force, w(0.0))
    n_pull = w(max(float((s > 0).sum()), 1.0))
    n_push = w(max(float((s < 0).sum()), 1.0))
    scale = norm_scale * np.where(
        s > 0, s * (w(1.0) / n_pull), s * (w(1.0) / n_push))
    scale_sum = scale.sum()
    moved = flat[me] + (scale @ flat - flat[me] * scale_sum)
    noise = laplace(seed, offset, b * flat_c + np.arange(flat_c), dtype, w)
    if q > 1:
      per_dim = noise.reshape(q, dc)
      maxabs = np.maximum(np.abs(per_dim).max(axis=0), w(1e-12))
      noise = (per_dim / maxabs[None, :]).reshape(flat_c)
    else:
      noise = np.where(noise >= 0.0, w(1.0), w(-1.0))
    out_cont[b] = (moved + noise * perts[me]).reshape(q, dc)
    for jd in range(flat_k):
      size = int(cat_sizes[jd % dcat])
      logit_same = _log(p_same, w)
      logit_diff = _log((w(1.0) - p_same) / max(w(size) - w(1.0), w(1e-9)),
                        w)
      cur = int(cats[me, jd])
      pert_noise = laplace(seed, offset ^ TAG_CAT_NOISE,
                           b * flat_k + jd, dtype, w) * cat_factor * perts[me]
      c = np.arange(size)
      logits = np.array([scale[cats[:, jd] == cc].sum() for cc in c],
                        dtype=w)
      logits = logits + logit_diff
      logits[cur] += -scale_sum + logit_same - logit_diff
      logits = logits + pert_noise
      u = uniform(seed, offset ^ TAG_GUMBEL, (b * flat_k + jd) * max_cat + c,
                  dtype).astype(w)
      vals = logits + -np.log(-np.log(np.maximum(u, w(1e-20))))
      all_vals[b, jd, :size] = vals
      order = np.sort(vals)
      if size > 1:
        margin = min(margin, float(order[-1] - order[-2]))
      out_cat[b, jd // dcat, jd % dcat] = int(np.argmax(vals))
  if return_vals:
    return out_cont, out_cat, margin, all_vals
  return out_cont, out_cat, margin


def update(pool_cont, pool_cat, rewards, perts, batch_cont, batch_cat,
           batch_rewards, cat_sizes, best_reward: float, offset: int,
           n_batches: int, seed: int, cfg: Config, dtype=np.float64):
  """In-place update of copies; returns the new state and row kinds.

  All arrays hold `dtype` values (q >= 1). `seed` is the update kernel's
  seed (the strategy passes seed ^ UPDATE_SEED_XOR). Returns (pool_cont,
  pool_cat, rewards, perts, new_best, kinds) with kinds[i] in
  {'improved', 'penalised', 'dead'}.
  """
  pool_cont, pool_cat = pool_cont.astype(dtype), pool_cat.copy()
  rewards, perts = rewards.astype(dtype), perts.astype(dtype)
  batch_cont = batch_cont.astype(dtype)
  batch_rewards = batch_rewards.astype(dtype)
  batch_size, q, dc = batch_cont.shape
  dcat = batch_cat.shape[2]
  flat_c, flat_k = q * dc, q * dcat
  penalize_factor = dtype(cfg.penalize_factor)
  lower_bound = dtype(cfg.perturbation_lower_bound)
  start = (offset % n_batches) * batch_size
  new_best = max(dtype(best_reward), batch_rewards.max())
  kinds = []
  for i in range(batch_size):
    me = start + i
    improved = batch_rewards[i] > rewards[me]
    pert = perts[me] if improved else perts[me] * penalize_factor
    reward = batch_rewards[i] if improved else rewards[me]
    dead = pert < lower_bound and reward != new_best
    if improved:
      pool_cont[me] = batch_cont[i]
      pool_cat[me] = batch_cat[i]
    if dead:
      pool_cont[me] = uniform(seed, offset ^ TAG_REFILL_CONT,
                              me * flat_c + np.arange(flat_c),
                              dtype).reshape(q, dc)
      for j in range(flat_k):
        u = uniform(seed, offset ^ TAG_REFILL_CAT, me * flat_k + j, dtype)
        size = int(cat_sizes[j % dcat])
        pool_cat[me, j // dcat, j % dcat] = min(int(u * dtype(size)),
                                                size - 1)
      reward = dtype(-math.inf)
      pert = dtype(cfg.perturbation)
    rewards[me] = reward
    perts[me] = pert
    kinds.append('dead' if dead else
                 'improved' if improved else 'penalised')
  return pool_cont, pool_cat, rewards, perts, float(new_best), kinds
