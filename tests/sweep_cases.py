"""Cases, fp64 oracle glue and child entry point for the Eagle sweep megakernel.

`ext.eagle_sweep` (eagle_sweep.hip) can be called directly with
`iterations=1` on any state, and afterwards every intermediate of that
iteration still sits in a tensor the caller passed in: `out_cont` (the
candidates), `k_ws`, `mu_ws`, `dist_ws`, `var_ws[:, :T]` (tile partials),
`var_ws[:, T]` (the reduced quadform) and the new pool state. So each phase
is checked against fp64 starting from the kernel's OWN output of the phase
before; no multi-iteration fp64 trajectory (which diverges at the first
accept/reject tie) is needed.

A case joins a pool state (`eagle_f64_oracle.steady_pool`, rounded to fp32)
with the well-conditioned synthetic scorer operands of
`scorer_cases.make_case`, and then ADJUSTS the state so that one iteration
provably reaches every Phase C outcome: the visited rows get rewards far
below (LOW) or far above (HIGH, BEST) anything the scorer can return, so
that no row sits within tolerance of its accept/reject threshold and the
GPU test can demand the kind of EVERY row. tests/test_sweep_cases.py checks
all of that with the oracle alone.

Shared by tests/test_sweep_kernel.py (GPU), tests/test_sweep_cases.py (CPU
self-check) and the child process (`python -m sweep_cases`) that runs the
sweep under VIZIER_AMD_SWEEP_GRID, a static read once per process.
"""

import argparse
import dataclasses
import functools
import sys
import types
from typing import Dict, List, Optional

import numpy as np
import torch

import eagle_f64_oracle as oracle
import scorer_cases as sc

F32 = np.float32

STRATEGY_SEED = 2024
# EI / PI threshold; differs from COEF so that a swap of the two shows.
BEST_VALUE = 0.9

# Rewards of the adjusted rows. The scorer returns |score| of a few units,
# or -1e4 - dist under the trust-region penalty; "far" is asserted by the
# CPU self-check as > 100 x the score tolerance from the fp64 score range.
LOW, HIGH, BEST = -3.0e4, 2.0e4, 3.0e4
STEP = 100.0            # spacing of the adjusted rewards: all distinct
# One penalty takes this under perturbation_lower_bound = 7e-5:
# 8e-5 is in [7e-5, 7e-5 / 0.7).
DEAD_PERT = 8e-5
# Perturbation of the trust-region "near" rows: 0.16 * 0.7^8 < 0.01.
TR_PERT = 0.16 * 0.7 ** 8
# Half-width of the training-row cluster of the trust-region variant.
TR_CLUSTER = 0.01

# name -> (pool, batch, dc, n); the smallest shape that reaches its branch.
CASES: Dict[str, tuple] = {
    'base': (50, 25, 4, 63),          # one partial tile, two batches
    'tile-64': (50, 25, 3, 64),       # exact tile
    'tile-65': (50, 25, 3, 65),       # 1-row second tile (ilen != 64)
    # The launcher's default grid is tiles clamped to [64, 128]: 100 tiles
    # get 100 workgroups, so B-stride takes its second trip of `tile += G`
    # only under a grid override (GRIDS); B-trip2 is the smallest n that
    # takes it at the default grid (144 tiles > 128).
    'B-stride': (100, 25, 5, 600),    # 100 tiles > 64 workgroups
    'B-trip2': (100, 25, 5, 710),     # 144 tiles > 128 workgroups
    'B2-stride': (100, 25, 5, 1100),  # 324 tiles > 256 threads
    'single-batch': (25, 25, 2, 130),
    'max-batch': (128, 32, 6, 200),   # MAX_POOL, VZ_QF_QMAX
    'b1': (8, 1, 3, 70),              # one candidate
    'stage-64': (128, 32, 64, 130),   # pool * dc == 8192: staged in LDS
    'stage-65': (128, 32, 65, 130),   # 8320: read through cload
    'dc-cap': (8, 4, 512, 70),        # xq_lds full
    'large-n': (50, 25, 3, 4100),     # 4225 tiles; standalone: SGEMM
}
ACQ_CASES = ('base', 'B-stride')       # every acquisition runs on these
TR_CASES = ('base', 'B-stride')
GRID_CASES = ('base', 'B-stride', 'max-batch')
GRIDS = (1, 7, 200)
# A full set of roles needs 2 low + 2 high + 2 dead + best + -inf rows.
FULL_ROLES_BATCH = 8

# Roles of the finite visited rows, in row order; alternating after these.
_ROLE_SEQ = ('dead', 'low', 'best', 'high', 'low', 'dead', 'high')


@dataclasses.dataclass
class SweepCase:
  name: str
  pool: int
  batch: int
  dc: int
  n: int
  seed: int                 # the strategy seed (suggest stream)
  tr: bool
  pool_cont: np.ndarray     # (pool, dc) fp32
  rewards: np.ndarray       # (pool,)    fp32
  perts: np.ndarray         # (pool,)    fp32
  best: np.float32
  x: torch.Tensor           # (n, dc) fp32
  ls: torch.Tensor          # (dc,)   fp32
  alpha: torch.Tensor       # (n,)    fp32
  M: torch.Tensor           # (n, n)  fp32, passed as K^-1
  roles: List[str]          # per visited row: low/high/dead/best/ninf
  near: List[int]           # trust-region variant: the two "near" rows

  @property
  def n_batches(self) -> int:
    return self.pool // self.batch

  @property
  def it_start(self) -> int:
    """offset_for of test_eagle_kernels.py: batch_start > 0 whenever there
    are two batches."""
    return 3 * self.n_batches - 1

  @property
  def start(self) -> int:
    return (self.it_start % self.n_batches) * self.batch

  @property
  def seed_update(self) -> int:
    return self.seed ^ oracle.UPDATE_SEED_XOR

  @property
  def tiles(self) -> int:
    t = (self.n + 63) // 64
    return t * t

  def full_iterations(self) -> int:
    """Every firefly is visited twice, and a restarted one moves again."""
    return 2 * self.n_batches + 1


def _pool3(a: np.ndarray) -> np.ndarray:
  return a[:, None, :]


def _no_cat(rows: int) -> np.ndarray:
  return np.zeros((rows, 1, 0), dtype=np.int64)


def oracle_candidates(case: SweepCase, arith=np.float64) -> np.ndarray:
  """(batch, dc) candidates of `oracle.suggest` on the pre-state."""
  out = oracle.suggest(
      _pool3(case.pool_cont), _no_cat(case.pool), case.rewards, case.perts,
      [], case.it_start, case.n_batches, case.batch, case.seed,
      oracle.Config(), dtype=F32, arith=arith)[0]
  return out[:, 0, :]


def make_sweep_case(pool: int, batch: int, dc: int, n: int, seed: int,
                    tr: bool = False, new_best: bool = False,
                    name: str = '') -> SweepCase:
  """Inputs of one direct `eagle_sweep` call; see the module docstring.

  Roles of the visited rows (rows batch_start .. batch_start + batch):
    low    reward LOW - k STEP: any candidate improves it
    high   reward HIGH + k STEP: no candidate does; penalised
    dead   high, perturbation DEAD_PERT: the penalty takes it under the
           lower bound, so it is restarted
    best   reward BEST = best_reward, perturbation DEAD_PERT: penalised
           under the bound, but exempt from the restart
    ninf   a -inf reward of steady_pool: my_reward = -inf
  A batch too small for all of them (FULL_ROLES_BATCH) takes the first of
  _ROLE_SEQ that fit; then `best` is held by an unvisited row. With
  `new_best` every finite reward of the pool is far BELOW the score range
  instead, so every visited row improves and best_reward is new. With `tr`
  two low rows share one position and a small perturbation, and x is a
  3-row cluster at their candidates with every other row >= 1 away.
  """
  assert pool % batch == 0 and not (tr and new_best)
  cont, _, rewards, perts = oracle.steady_pool(pool, 1, dc, [], seed)
  cont = cont[:, 0, :].astype(F32)
  rewards, perts = rewards.astype(F32), perts.astype(F32)
  assert int(np.isinf(rewards).sum()) == 3
  scorer = sc.make_case(batch, n, dc, seed)
  case = SweepCase(
      name=name or f'{pool}x{batch}x{dc}x{n}', pool=pool, batch=batch,
      dc=dc, n=n, seed=STRATEGY_SEED, tr=tr, pool_cont=cont,
      rewards=rewards, perts=perts, best=F32(BEST), x=scorer.x.clone(),
      ls=scorer.ls, alpha=scorer.alpha, M=scorer.M, roles=[], near=[])
  start = case.start
  visited = np.arange(start, start + batch)
  outside = np.setdiff1d(np.arange(pool), visited)

  def swap(a, b):
    rewards[[a, b]] = rewards[[b, a]]

  def infs(rows):
    return [int(r) for r in rows if np.isinf(rewards[r])]

  def finite(rows):
    return [int(r) for r in rows if np.isfinite(rewards[r])]

  # The three -inf rewards stay; at least one inside the visited batch (if
  # it has room for the other roles too) and at least one outside it.
  if batch >= 4 and not infs(visited):
    swap(infs(outside)[0], start + 4 if batch > 4 else start + batch - 1)
  if batch < 4:
    for r in infs(visited):
      swap(r, finite(outside)[0])
  if len(outside) and not infs(outside):
    swap(infs(visited)[-1], finite(outside)[0])

  roles = {}
  for k, r in enumerate(finite(visited)):
    role = (_ROLE_SEQ[k] if k < len(_ROLE_SEQ)
            else ('low' if k % 2 else 'high'))
    roles[r] = 'low' if new_best else role
    if roles[r] == 'low':
      rewards[r] = LOW - STEP * k
    elif roles[r] == 'best':
      rewards[r] = BEST
    else:
      rewards[r] = HIGH + STEP * k
    if roles[r] in ('dead', 'best'):
      perts[r] = DEAD_PERT
  if new_best:
    for k, r in enumerate(finite(outside)):
      rewards[r] = LOW - STEP * (batch + k)
    case.best = F32(rewards[np.isfinite(rewards)].max())
  elif 'best' not in roles.values():
    rewards[finite(outside)[0]] = BEST
  case.roles = [roles.get(int(r), 'ninf') for r in visited]
  assert float(rewards[np.isfinite(rewards)].max()) == float(case.best)

  if tr:
    low = [int(r) for r in visited if roles.get(int(r)) == 'low'][:2]
    cont[low[1]] = cont[low[0]]
    perts[low] = TR_PERT
    case.near = [r - start for r in low]
    cand = oracle_candidates(case)
    center = 0.5 * (cand[case.near[0]] + cand[case.near[1]])
    x = 2.0 + 0.5 * case.x.double().numpy()
    x[0], x[1], x[2] = center, center + TR_CLUSTER, center - TR_CLUSTER
    case.x = torch.from_numpy(x.astype(F32))
  return case


@functools.lru_cache(maxsize=None)
def sweep_case(name: str, variant: str = '') -> SweepCase:
  """The (shared, never mutated) case of a name; variant '', 'tr' or
  'newbest'."""
  pool, batch, dc, n = CASES[name]
  assert variant in ('', 'tr', 'newbest'), variant
  return make_sweep_case(
      pool, batch, dc, n, seed=pool + 3 * dc + n, tr=variant == 'tr',
      new_best=variant == 'newbest',
      name=name + ('-' + variant if variant else ''))


def case_by_id(case_id: str) -> SweepCase:
  """'base', 'base-tr', 'base-newbest', 'tile-64', ..."""
  for variant in ('tr', 'newbest'):
    if case_id.endswith('-' + variant):
      return sweep_case(case_id[:-len(variant) - 1], variant)
  return sweep_case(case_id)


# -- the fp64 oracle of one iteration -----------------------------------------


def dist_f32(xq: np.ndarray, x: np.ndarray) -> np.ndarray:
  """min over rows of max_j |fl32(xq_j - x_j)|: the kernel's distance, whose
  only rounding is the fp32 subtraction (max, min and abs are exact)."""
  diff = np.abs(xq.astype(F32)[:, None, :] - x.astype(F32)[None, :, :])
  assert diff.dtype == F32
  return diff.max(-1).min(-1)


def oracle_iteration(case: SweepCase, acq: str, coef: float,
                     best_value: float, tr_radius: float, observed,
                     dtype=torch.float64):
  """One iteration in fp64, staged from the kernel's own candidates.

  observed.out_cont holds the kernel's candidates (batch, dc) as fp32
  values. Returns a namespace with
    cand64, cand32       oracle.suggest on the pre-state, fp64 / fp32 arith
    k, mean, quad, sd, dist, score, penalised   from observed.out_cont
    pool, rewards, perts, best, kinds   oracle.update fed those scores
  `dtype=torch.float32` evaluates the scorer stage in fp32 torch arithmetic
  instead (the CPU self-check's threshold-margin test).
  """
  from vizier_amd._src.ops import dispatch
  code = dispatch.ACQ_CODES[acq]
  out_cont = np.asarray(observed.out_cont, dtype=F32)
  xq = torch.from_numpy(out_cont).to(dtype)
  k = sc.kvec_direct(xq, case.x.to(dtype), case.ls.to(dtype))
  ref = sc.posterior_from_k(k, case.alpha.to(dtype), case.M.to(dtype))
  dist = sc.min_linf_dist(xq, case.x.to(dtype), [0] * case.dc)
  score = sc.acquisition(code, ref.mean, ref.sd, coef, best_value)
  penalised = dist > tr_radius if 0.0 < tr_radius <= 0.5 else \
      torch.zeros_like(dist, dtype=torch.bool)
  score = torch.where(penalised, -1e4 - dist, score)
  post = oracle.update(
      _pool3(case.pool_cont), _no_cat(case.pool), case.rewards, case.perts,
      _pool3(out_cont), _no_cat(case.batch), score.double().numpy(), [],
      float(case.best), case.it_start, case.n_batches, case.seed_update,
      oracle.Config(), dtype=F32)
  return types.SimpleNamespace(
      cand64=oracle_candidates(case, np.float64),
      cand32=oracle_candidates(case, F32),
      k=k, mean=ref.mean, quad=ref.quad, sd=ref.sd, dist=dist, score=score,
      penalised=penalised, pool=post[0][:, 0, :], rewards=post[2],
      perts=post[3], best=post[4], kinds=post[5])


def observed_kinds(case: SweepCase, rewards: np.ndarray,
                   perts: np.ndarray) -> List[str]:
  """Kinds of the visited rows read off a post-state: a restart leaves
  -inf, an accepted move leaves the perturbation as it was, and a penalty
  multiplies it by 0.7."""
  kinds = []
  for r in range(case.start, case.start + case.batch):
    if np.isneginf(rewards[r]):
      kinds.append('dead')
    elif perts[r] == case.perts[r]:
      kinds.append('improved')
    else:
      kinds.append('penalised')
  return kinds


# -- GPU runs -----------------------------------------------------------------


def _cfg_args(cfg: oracle.Config):
  return (cfg.visibility, cfg.gravity, cfg.negative_gravity,
          cfg.normalization_scale, cfg.penalize_factor,
          cfg.perturbation_lower_bound, cfg.perturbation)


@dataclasses.dataclass
class SweepCall:
  """The 35 positional arguments of `ext.eagle_sweep`, by name, so that a
  test can replace one (`dataclasses.replace`)."""
  pool_cont: torch.Tensor
  rewards: torch.Tensor
  perts: torch.Tensor
  best: torch.Tensor
  iter_t: torch.Tensor
  barrier: torch.Tensor
  x: torch.Tensor
  inv_ls: torch.Tensor
  alpha: torch.Tensor
  M: torch.Tensor
  out_cont: torch.Tensor
  k_ws: torch.Tensor
  mu_ws: torch.Tensor
  dist_ws: torch.Tensor
  var_ws: torch.Tensor
  n_batches: int
  batch: int
  pool: int
  it_start: int
  iterations: int
  acq: int
  coef: float
  best_value: float
  tr_radius: float
  seed: int
  seed_update: int

  def args(self):
    return (self.pool_cont, self.rewards, self.perts, self.best, self.iter_t,
            self.barrier, self.x, self.inv_ls, self.alpha, self.M,
            self.out_cont, self.k_ws, self.mu_ws, self.dist_ws, self.var_ws,
            self.n_batches, self.batch, self.pool, self.it_start,
            self.iterations, *_cfg_args(oracle.Config()), self.seed,
            self.seed_update, sc.AMP * sc.AMP, sc.MEAN_C, self.acq,
            self.coef, self.best_value, self.tr_radius)

  def state(self):
    return (self.pool_cont, self.rewards, self.perts, self.best)


def sweep_call(case: SweepCase, iterations: int, acq: str = 'ucb',
               coef: float = sc.COEF, best_value: float = BEST_VALUE,
               tr_radius: float = 0.0, device='cuda') -> SweepCall:
  """A valid call on fresh device copies of the case. The workspaces start
  as NaN, so an entry no phase wrote shows."""
  from vizier_amd._src.ops import dispatch

  def dev(a):
    return torch.as_tensor(np.array(a)).to(device)

  def nan(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float32,
                      device=device)
  iter_t = torch.zeros(12, dtype=torch.long, device=device)
  iter_t[0], iter_t[1] = case.it_start, case.it_start - 1
  ls = case.ls.to(device)
  return SweepCall(
      pool_cont=dev(case.pool_cont), rewards=dev(case.rewards),
      perts=dev(case.perts), best=dev([case.best]), iter_t=iter_t,
      barrier=torch.zeros(2, dtype=torch.int32, device=device),
      x=case.x.to(device), inv_ls=(1.0 / ls).contiguous(),
      alpha=case.alpha.to(device), M=case.M.to(device),
      out_cont=nan(case.batch, case.dc), k_ws=nan(case.batch, case.n),
      mu_ws=nan(case.batch), dist_ws=nan(case.batch),
      var_ws=nan(case.batch, case.tiles + 1), n_batches=case.n_batches,
      batch=case.batch, pool=case.pool, it_start=case.it_start,
      iterations=iterations, acq=dispatch.ACQ_CODES[acq], coef=coef,
      best_value=best_value, tr_radius=tr_radius, seed=case.seed,
      seed_update=case.seed_update)


def run_sweep(ext, case: SweepCase, iterations: int, **kwargs) -> SweepCall:
  """One `ext.eagle_sweep` call; returns the call with its tensors (state
  and workspaces) as the kernel left them. `grid` is the grid it used."""
  call = sweep_call(case, iterations, **kwargs)
  call.grid = ext.eagle_sweep(*call.args())
  torch.cuda.synchronize()
  return call


def compose_step_kernels(ext, case: SweepCase, iterations: int,
                         acq: str = 'ucb', coef: float = sc.COEF,
                         best_value: float = BEST_VALUE,
                         tr_radius: float = 0.0, device='cuda'):
  """The same iterations as direct calls of the standalone bindings, as the
  strategy makes them: eagle_suggest -> posterior_scores_chunked ->
  eagle_update with an all-false onehot and the seeds `seed` and
  `seed ^ 0xABCDEF`. Returns a namespace with the full state, `iter_t` and
  `dead`, the number of restarts over all iterations."""
  from vizier_amd._src.ops import dispatch
  cfg = oracle.Config()
  call = sweep_call(case, iterations, acq, coef, best_value, tr_radius,
                    device)
  pool3 = call.pool_cont.view(case.pool, 1, case.dc)
  pool_cat = torch.zeros(case.pool, 1, 0, dtype=torch.long, device=device)
  cat_sizes = torch.zeros(0, dtype=torch.long, device=device)
  out_cont = torch.empty(case.batch, 1, case.dc, dtype=torch.float32,
                         device=device)
  out_cat = torch.zeros(case.batch, 1, 0, dtype=torch.long, device=device)
  onehot = torch.zeros(case.dc, dtype=torch.uint8, device=device)
  ls = case.ls.to(device)
  iter_t = call.iter_t
  iter_t[:2] = case.it_start        # as the strategy aligns it
  dead = 0
  for it in range(case.it_start, case.it_start + iterations):
    ext.eagle_suggest(
        pool3, pool_cat, call.rewards, call.perts, cat_sizes, iter_t,
        case.n_batches, case.batch, cfg.visibility, cfg.gravity,
        cfg.negative_gravity, cfg.normalization_scale, cfg.cat_factor,
        cfg.p_same, case.seed, out_cont, out_cat, 0)
    scores = ext.posterior_scores_chunked(
        out_cont[:, 0, :], call.x, ls, sc.AMP, sc.MEAN_C, call.alpha, call.M,
        onehot, dispatch.ACQ_CODES[acq], coef, best_value, tr_radius)
    ext.eagle_update(
        pool3, pool_cat, call.rewards, call.perts, out_cont, out_cat,
        scores, cat_sizes, call.best, iter_t, case.n_batches,
        cfg.penalize_factor, cfg.perturbation_lower_bound, cfg.perturbation,
        case.seed_update)
    start = (it % case.n_batches) * case.batch
    # A visited row ends an iteration with -inf only through a restart.
    dead += int(torch.isneginf(
        call.rewards[start:start + case.batch]).sum())
  torch.cuda.synchronize()
  return types.SimpleNamespace(
      pool_cont=call.pool_cont, rewards=call.rewards, perts=call.perts,
      best=call.best, iter_t=iter_t, dead=dead)


# -- child process: VIZIER_AMD_SWEEP_GRID ---------------------------------------


def child_main(argv: Optional[List[str]] = None) -> int:
  """Runs the listed cases through `ext.eagle_sweep` (UCB) and writes the
  final state of each to an .npz. The parent sets VIZIER_AMD_SWEEP_GRID in
  the environment and does all comparing."""
  p = argparse.ArgumentParser()
  p.add_argument('--out', required=True)
  p.add_argument('--cases', required=True, help='comma-separated case ids')
  p.add_argument('--iterations', required=True,
                 help='comma-separated, one per case')
  args = p.parse_args(argv)
  from vizier_amd._src.ops import dispatch
  ext = dispatch.require_ext()
  ids = args.cases.split(',')
  iterations = [int(v) for v in args.iterations.split(',')]
  assert len(ids) == len(iterations), (ids, iterations)
  out = {}
  for case_id, its in zip(ids, iterations):
    call = run_sweep(ext, case_by_id(case_id), its)
    out[f'{case_id}/grid'] = np.int64(call.grid)
    out[f'{case_id}/pool_cont'] = call.pool_cont.cpu().numpy()
    out[f'{case_id}/rewards'] = call.rewards.cpu().numpy()
    out[f'{case_id}/perts'] = call.perts.cpu().numpy()
    out[f'{case_id}/best'] = call.best.cpu().numpy()
    out[f'{case_id}/iter'] = call.iter_t[:2].cpu().numpy()
  np.savez(args.out, **out)
  return 0


if __name__ == '__main__':
  sys.exit(child_main())
