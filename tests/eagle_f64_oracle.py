"""NumPy fp64 oracle of the fp64 Eagle kernels (eagle_step_f64.hip).

splitmix64 on np.uint64 with the constants of csrc/common.h, the widened
24-bit uniform, Laplace and Gumbel in double, and the suggest / update
formulas of vizier_amd/_src/algorithms/optimizers/eagle.py as the kernels
evaluate them. Shared by tests/test_fp64_kernels.py (GPU) and
tests/test_fp64_dispatch.py (CPU: hard-coded splitmix64 values).
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


def uniform(seed: int, offset: int, idx) -> np.ndarray:
  """((h >> 40) + 0.5) / 2^24 with h = mix(seed ^ mix(offset ^ idx))."""
  idx = np.asarray(idx, dtype=np.uint32).astype(_U64)
  h = splitmix64(_U64(seed) ^ splitmix64(_U64(offset) ^ idx))
  return ((h >> _U64(40)).astype(np.float64) + 0.5) / 16777216.0


def laplace(seed: int, offset: int, idx) -> np.ndarray:
  u = uniform(seed, offset, idx) - 0.5
  a = np.minimum(np.abs(u), 0.499999)
  return np.where(u >= 0.0, -1.0, 1.0) * np.log1p(-2.0 * a)


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


def suggest(pool_cont, pool_cat, rewards, perts, cat_sizes, offset: int,
            n_batches: int, batch_size: int, seed: int, cfg: Config):
  """q = 1. pool_cont (P, 1, Dc) f64, pool_cat (P, 1, Dcat) int64.

  Returns (out_cont (B, 1, Dc), out_cat (B, 1, Dcat), margin): margin is
  the smallest gap between the best and second-best `logit + gumbel` over
  every categorical entry (inf without categoricals).
  """
  pool_size, q, dc = pool_cont.shape
  assert q == 1
  dcat = pool_cat.shape[2]
  n_features = dc + dcat
  max_cat = int(max(cat_sizes)) if dcat else 0
  flat = pool_cont.reshape(pool_size, dc)
  cats = pool_cat.reshape(pool_size, dcat)
  start = (offset % n_batches) * batch_size
  out_cont = np.empty((batch_size, 1, dc))
  out_cat = np.empty((batch_size, 1, dcat), dtype=np.int64)
  margin = math.inf
  for b in range(batch_size):
    me = start + b
    diff = flat[me][None, :] - flat
    d2 = (diff * diff).sum(-1) + (cats != cats[me][None, :]).sum(-1)
    with np.errstate(invalid='ignore'):   # -inf - -inf: s is zeroed below
      direction = np.where(rewards - rewards[me] >= 0.0, cfg.gravity,
                           -cfg.negative_gravity)
    force = np.exp(-cfg.visibility * d2 / n_features * 10.0)
    s = np.where(np.isfinite(rewards), direction * force, 0.0)
    n_pull = max(float((s > 0).sum()), 1.0)
    n_push = max(float((s < 0).sum()), 1.0)
    scale = cfg.normalization_scale * np.where(
        s > 0, s * (1.0 / n_pull), s * (1.0 / n_push))
    scale_sum = scale.sum()
    moved = flat[me] + (scale @ flat - flat[me] * scale_sum)
    noise = laplace(seed, offset, b * dc + np.arange(dc))
    sign = np.where(noise >= 0.0, 1.0, -1.0)
    out_cont[b, 0] = moved + sign * perts[me]
    for jd in range(dcat):
      size = int(cat_sizes[jd])
      logit_same = math.log(cfg.p_same)
      logit_diff = math.log((1.0 - cfg.p_same) / max(size - 1.0, 1e-9))
      cur = int(cats[me, jd])
      pert_noise = float(laplace(seed, offset ^ TAG_CAT_NOISE,
                                 b * dcat + jd)) * cfg.cat_factor * perts[me]
      c = np.arange(size)
      logits = np.array([scale[cats[:, jd] == cc].sum() for cc in c])
      logits = logits + logit_diff
      logits[cur] += -scale_sum + logit_same - logit_diff
      logits = logits + pert_noise
      u = uniform(seed, offset ^ TAG_GUMBEL, (b * dcat + jd) * max_cat + c)
      vals = logits + -np.log(-np.log(np.maximum(u, 1e-20)))
      order = np.sort(vals)
      if size > 1:
        margin = min(margin, float(order[-1] - order[-2]))
      out_cat[b, 0, jd] = int(np.argmax(vals))
  return out_cont, out_cat, margin


def update(pool_cont, pool_cat, rewards, perts, batch_cont, batch_cat,
           batch_rewards, cat_sizes, best_reward: float, offset: int,
           n_batches: int, seed: int, cfg: Config):
  """In-place update of copies; returns the new state and row kinds.

  `seed` is the update kernel's seed (the strategy passes
  seed ^ UPDATE_SEED_XOR). Returns (pool_cont, pool_cat, rewards, perts,
  new_best, kinds) with kinds[i] in {'improved', 'penalised', 'dead'}.
  """
  pool_cont, pool_cat = pool_cont.copy(), pool_cat.copy()
  rewards, perts = rewards.copy(), perts.copy()
  batch_size, q, dc = batch_cont.shape
  assert q == 1
  dcat = batch_cat.shape[2]
  start = (offset % n_batches) * batch_size
  new_best = max(best_reward, float(batch_rewards.max()))
  kinds = []
  for i in range(batch_size):
    me = start + i
    improved = batch_rewards[i] > rewards[me]
    pert = perts[me] if improved else perts[me] * cfg.penalize_factor
    reward = batch_rewards[i] if improved else rewards[me]
    dead = pert < cfg.perturbation_lower_bound and reward != new_best
    if improved:
      pool_cont[me] = batch_cont[i]
      pool_cat[me] = batch_cat[i]
    if dead:
      pool_cont[me, 0] = uniform(seed, offset ^ TAG_REFILL_CONT,
                                 me * dc + np.arange(dc))
      for j in range(dcat):
        u = float(uniform(seed, offset ^ TAG_REFILL_CAT, me * dcat + j))
        size = int(cat_sizes[j])
        pool_cat[me, 0, j] = min(int(u * size), size - 1)
      reward = -math.inf
      pert = cfg.perturbation
    rewards[me] = reward
    perts[me] = pert
    kinds.append('dead' if dead else
                 'improved' if improved else 'penalised')
  return pool_cont, pool_cat, rewards, perts, new_best, kinds
