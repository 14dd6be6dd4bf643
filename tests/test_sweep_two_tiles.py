"""The sweep megakernel under 512-thread workgroups (eagle_sweep.hip): phase
B runs two tiles per workgroup, one per half of 256 threads, and every other
phase runs the 256-thread arithmetic on half 0 while half 1 only takes the
barriers.

Every comparison is BITWISE. The reference is the standalone step kernels
for the same seeds (`eagle_suggest` -> `posterior_scores_chunked` ->
`eagle_update`, as `sweep_cases.compose_step_kernels` chains them), run for
the same iterations:

  state        `pool_cont`, `rewards`, `perts`, `best`, `iter_t[:2]` after
               `full_iterations()` (every pool batch visited twice)
  out_cont     the last iteration's candidates against `eagle_suggest`'s
  mu_ws        `fl(mu_ws + mean_c)` against the step scorer's mean
               (`posterior_mean_std`, the same k-vector kernel and tile
               quadform as `posterior_scores_chunked`)
  var_ws[:, T] `sqrt(max(amp2 - quad, 1e-12))`, in correctly rounded fp32,
               against the step scorer's standard deviation
  dist_ws      against the step scorer's distance

The step bindings do not hand out their k-vector or their tile partials, so
`k_ws` and `var_ws[:, :T]` of the last iteration are compared, bitwise, with
those of a ONE-iteration sweep launch started from the step kernels' state
before that iteration (fresh NaN workspaces): anything a launch carried
over from an earlier iteration, or a tile nobody wrote, shows. Their bits
are pinned to the step kernels through the rewards, which are the scores
computed from them.

The tests pin bits, not speed: they pass on the 256-thread kernel too.

Shapes `(pool, batch, dc, n)`, at the default grid clamp(tiles, 64, 128):

  n = 60     one partial tile, grid 64: no half 1 ever has a tile
  n = 576    81 tiles, grid 81: every half 1 idle
  n = 705    144 tiles, grid 128: half 1 has a tile in workgroups 0..15 only;
             the last tile row and column have length 1
  n = 1024   256 tiles: exactly one tile per half
  n = 1025   289 tiles: the second trip has 33 tiles for half 0, none for
             half 1; edge length 1
  n = 2049   1089 tiles > FOLD_MAX_TILES: phase B2 and its barrier
crossed sparingly with batch 1 / 7 / 25 / 32, dc 1 / 20 / 21 and the two
legacy pool modes (pool 128 with dc 33 and dc 65: phase A's staging and
phase C run under eight waves).
"""

import dataclasses
import functools
import types

import numpy as np
import pytest
import torch

import eagle_f64_oracle as oracle
import scorer_cases as sc
import sweep_cases as sw

pytestmark = pytest.mark.gpu

CASES = {
    'one-partial-tile': (50, 25, 20, 60),
    'half1-idle-batch-7': (14, 7, 4, 576),
    'ragged-705-dc-21': (50, 25, 21, 705),
    'batch-1-dc-1': (8, 1, 1, 705),
    'one-tile-per-half': (50, 25, 20, 1024),
    'trip2-1025-batch-32': (64, 32, 4, 1025),
    'not-folded-2049': (9, 3, 2, 2049),
    'legacy-staged': (128, 32, 33, 705),
    'legacy-unstaged': (128, 32, 65, 130),
}


@pytest.fixture(scope='module')
def ext():
  from vizier_amd._src.ops import dispatch
  return dispatch.require_ext()  # Fails loudly if the .so is missing.


@functools.lru_cache(maxsize=None)
def _case(name, seed_shift=0):
  pool, batch, dc, n = CASES[name]
  return sw.make_sweep_case(pool, batch, dc, n,
                            seed=pool + 3 * dc + n + seed_shift, name=name)


def _step_reference(ext, case, iterations):
  """`iterations` of the step kernels, as `sw.compose_step_kernels` runs
  them. Returns the final state, the state before the last iteration, and
  the last iteration's candidates with the step scorer's mean, standard
  deviation and distance for them."""
  from vizier_amd._src.ops import dispatch
  cfg = oracle.Config()
  call = sw.sweep_call(case, iterations)
  pool3 = call.pool_cont.view(case.pool, 1, case.dc)
  pool_cat = torch.zeros(case.pool, 1, 0, dtype=torch.long, device='cuda')
  cat_sizes = torch.zeros(0, dtype=torch.long, device='cuda')
  out_cont = torch.empty(case.batch, 1, case.dc, dtype=torch.float32,
                         device='cuda')
  out_cat = torch.zeros(case.batch, 1, 0, dtype=torch.long, device='cuda')
  onehot = torch.zeros(case.dc, dtype=torch.uint8, device='cuda')
  ls = case.ls.to('cuda')
  iter_t = call.iter_t
  iter_t[:2] = case.it_start
  before = None
  for k in range(iterations):
    if k == iterations - 1:
      before = [t.clone() for t in call.state()]
    ext.eagle_suggest(
        pool3, pool_cat, call.rewards, call.perts, cat_sizes, iter_t,
        case.n_batches, case.batch, cfg.visibility, cfg.gravity,
        cfg.negative_gravity, cfg.normalization_scale, cfg.cat_factor,
        cfg.p_same, case.seed, out_cont, out_cat, 0)
    scores = ext.posterior_scores_chunked(
        out_cont[:, 0, :], call.x, ls, sc.AMP, sc.MEAN_C, call.alpha, call.M,
        onehot, dispatch.ACQ_CODES['ucb'], sc.COEF, sw.BEST_VALUE, 0.0)
    ext.eagle_update(
        pool3, pool_cat, call.rewards, call.perts, out_cont, out_cat,
        scores, cat_sizes, call.best, iter_t, case.n_batches,
        cfg.penalize_factor, cfg.perturbation_lower_bound, cfg.perturbation,
        case.seed_update)
  mean, sd, dist = ext.posterior_mean_std(
      out_cont[:, 0, :], call.x, ls, sc.AMP, sc.MEAN_C, call.alpha, call.M,
      onehot)
  torch.cuda.synchronize()
  return types.SimpleNamespace(
      pool_cont=call.pool_cont, rewards=call.rewards, perts=call.perts,
      best=call.best, iter_t=iter_t, before=before,
      out_cont=out_cont[:, 0, :].clone(), mean=mean, sd=sd, dist=dist)


def _assert_state_equal(got, want, tag):
  for key in ('pool_cont', 'rewards', 'perts', 'best'):
    assert torch.equal(getattr(got, key), getattr(want, key)), (tag, key)
  assert got.iter_t[:2].tolist() == want.iter_t[:2].tolist(), tag


def _assert_workspaces_equal(got, want, tag):
  for key in ('out_cont', 'k_ws', 'mu_ws', 'dist_ws', 'var_ws'):
    a, b = getattr(got, key), getattr(want, key)
    assert not bool(torch.isnan(a).any()), (tag, key)   # every entry written
    assert torch.equal(a, b), (tag, key)


def _assert_equals_steps(ext, case, got, iterations, tag):
  """`got`: a sweep of `iterations` from the case's initial state."""
  want = _step_reference(ext, case, iterations)
  _assert_state_equal(got, want, tag)
  assert torch.equal(got.out_cont, want.out_cont), (tag, 'out_cont')
  assert torch.equal(got.dist_ws, want.dist), (tag, 'dist_ws')
  f32 = np.float32
  mu = got.mu_ws.cpu().numpy()
  assert mu.dtype == f32
  assert np.array_equal(mu + f32(sc.MEAN_C), want.mean.cpu().numpy()), (
      tag, 'mu_ws')
  quad = got.var_ws[:, case.tiles].cpu().numpy()
  amp2 = f32(sc.AMP * sc.AMP)
  sd = np.sqrt(np.maximum(amp2 - quad, f32(1e-12)))
  assert sd.dtype == f32
  assert np.array_equal(sd, want.sd.cpu().numpy()), (tag, 'var_ws[:, T]')
  # The last iteration again, as a launch of its own on the step kernels'
  # state before it.
  one = sw.sweep_call(case, 1)
  for dst, src in zip(one.state(), want.before):
    dst.copy_(src)
  last = case.it_start + iterations - 1
  one = dataclasses.replace(one, it_start=last)
  one.iter_t[0], one.iter_t[1] = last, last - 1
  ext.eagle_sweep(*one.args())
  torch.cuda.synchronize()
  _assert_state_equal(one, want, (tag, 'one iteration'))
  _assert_workspaces_equal(got, one, tag)


@pytest.mark.parametrize('name', CASES)
def test_two_tile_sweep_equals_step_kernels(ext, name):
  case = _case(name)
  pool, batch, dc, n = CASES[name]
  if name == 'legacy-staged':
    assert 4096 < pool * dc <= 8192
  if name == 'legacy-unstaged':
    assert pool * dc > 8192
  if name == 'not-folded-2049':
    assert case.tiles > 1024
  its = case.full_iterations()
  got = sw.run_sweep(ext, case, its)
  assert got.grid == min(max(case.tiles, 64), 128)
  _assert_equals_steps(ext, case, got, its, name)
  assert not torch.equal(got.pool_cont.cpu(),
                         torch.from_numpy(case.pool_cont))


def test_two_launches_with_different_kinv(ext):
  """One tile per half: a K^-1 tile (or anything else of a launch) kept
  across launches of one process would show in the second and third."""
  first, second = _case('one-tile-per-half'), _case('one-tile-per-half', 1)
  assert not torch.equal(first.M, second.M)
  assert not torch.equal(first.alpha, second.alpha)
  its = first.full_iterations()
  for tag, case in (('first', first), ('second', second),
                    ('first again', first)):
    got = sw.run_sweep(ext, case, its)
    _assert_equals_steps(ext, case, got, its, tag)


def test_split_calls_equal_one_call(ext):
  """One sweep cut into two `eagle_sweep` calls on the same tensors, with
  `it_start` continuing and a zeroed barrier each, as
  test_sweep_resident.py does for the Eagle state."""
  case = _case('one-tile-per-half')
  its = case.full_iterations()
  whole = sw.run_sweep(ext, case, its)
  call = sw.sweep_call(case, 2)
  done = 0
  for chunk in (2, its - 2):
    step = dataclasses.replace(
        call, it_start=case.it_start + done, iterations=chunk,
        barrier=torch.zeros_like(call.barrier))
    ext.eagle_sweep(*step.args())
    done += chunk
  torch.cuda.synchronize()
  _assert_state_equal(call, whole, 'split')
  _assert_workspaces_equal(call, whole, 'split')
