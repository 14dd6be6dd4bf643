"""The Eagle sweep megakernel (eagle_sweep.hip) phase by phase against fp64.

`ext.eagle_sweep` is called directly with `iterations=1` on the adjusted
states of tests/sweep_cases.py; afterwards every intermediate of the
iteration sits in a tensor of the call, and each phase is checked against
fp64 starting from the kernel's OWN output of the phase before:

  candidates   out_cont against oracle.suggest, within the bound of
               test_eagle_kernels.py::test_eagle_suggest: 4 x (fp32-arith vs
               fp64-arith oracle), floored at 8 pool 2^-24 (1 + max|x|)
  k, mean,     from the kernel's candidates, within scorer_cases.TOL_FP32
  quad
  dist         BITWISE equal to min_rows max_j |fl32(xq_j - x_j)|. The fp64
               oracle holds the exact differences, which fp32 does not in
               general, so the bitwise reference is the oracle evaluated
               on fp32 differences (max, min and abs are exact); against
               the fp64 oracle the bound is that one rounding,
               2^-24 max|xq - x|.
  B2           var_ws[:, T] against the fp64 sum of the kernel's own tile
               partials var_ws[:, :T], within T 2^-24 sum|partials|
  Phase C      EVERY visited row has the kind oracle.update gives; pools,
               perturbations and unaccepted rewards bitwise, accepted
               rewards within acq_tolerance / TOL_PENALTY of the fp64 score
Then the whole state of a multi-iteration sweep is compared bitwise with
the standalone step kernels (N < 4096), with itself at other grid sizes
(fresh child processes: VIZIER_AMD_SWEEP_GRID is read once per process),
and, through the optimizer, with the hipGraph path for four acquisitions.

Largest observed / bound ratio per stage on the MI355X, with the case it
occurred in; `pytest -rA` prints the figure of every case (OBSERVED lines):

  candidates          0.015   dc-cap       1.2e-7 of 7.6e-6
  k                   0.011   B-stride     3.9e-7 of 3.4e-5
  mean                0.010   large-n      3.4e-7 of 3.4e-5
  quad                0.0055  stage-64     1.8e-7 of 3.4e-5
  dist vs fp64        0.47    stage-64     3.0e-8 of 6.3e-8 (bitwise vs fp32)
  B2 reduce           0.28    tile-65      5.3e-8 of 1.9e-7
  accepted rewards    0.0085  stage-64     (plain acquisition)
  penalised rewards   0.22    B-stride-tr  4.4e-4 of 2e-3
"""

import dataclasses
import os
import subprocess
import sys
import time
import types

import numpy as np
import pytest
import torch

import eagle_f64_oracle as oracle
import scorer_cases as sc
import sweep_cases as sw

pytestmark = pytest.mark.gpu

_TESTS = os.path.dirname(os.path.abspath(__file__))
_REPO = os.path.dirname(_TESTS)
F32 = np.float32
EPS = 2.0 ** -24


@pytest.fixture(scope='module')
def ext():
  from vizier_amd._src.ops import dispatch
  return dispatch.require_ext()  # Fails loudly if the .so is missing.


def _report(what, err, tol):
  print(f'OBSERVED {what}: err {err:.3e} (bound {tol:.3e})')
  assert err <= tol, (what, err, tol)


def _np(t):
  return t.detach().cpu().numpy()


# -- (a) one iteration, staged, against fp64 ------------------------------------

ONE_ITERATION = (
    [(case_id, 'ucb') for case_id in sw.CASES] +
    [(case_id, acq) for case_id in sw.ACQ_CASES
     for acq in sc.ACQ_NAMES if acq != 'ucb'] +
    [('base-newbest', 'ucb')])


def _check_iteration(ext, case, acq, tr_radius=0.0):
  """Runs one iteration and asserts every stage; returns (call, oracle)."""
  code = sc.ACQ_NAMES.index(acq)
  tag = f'{case.name} {acq} tr={tr_radius}'
  got = sw.run_sweep(ext, case, 1, acq=acq, tr_radius=tr_radius)
  if 'VIZIER_AMD_SWEEP_GRID' not in os.environ:
    assert 1 <= got.grid <= 128         # the launcher's cap
  out_cont = _np(got.out_cont)
  o = sw.oracle_iteration(case, acq, sc.COEF, sw.BEST_VALUE, tr_radius,
                          types.SimpleNamespace(out_cont=out_cont))
  start, batch, dc, T = case.start, case.batch, case.dc, case.tiles

  # Candidates.
  floor = 8.0 * case.pool * EPS * (1.0 + float(np.abs(case.pool_cont).max()))
  tol = max(4.0 * float(np.abs(o.cand32 - o.cand64).max()), floor)
  _report(f'{tag} candidates',
          float(np.abs(out_cont.astype(np.float64) - o.cand64).max()), tol)

  # Scorer stages, from the kernel's own candidates.
  _report(f'{tag} k', float((got.k_ws.cpu().double() - o.k).abs().max()),
          sc.TOL_FP32)
  _report(f'{tag} mean',
          float((got.mu_ws.cpu().double() + sc.MEAN_C - o.mean).abs().max()),
          sc.TOL_FP32)
  dist = _np(got.dist_ws)
  x = case.x.numpy()
  assert np.array_equal(dist, sw.dist_f32(out_cont, x)), tag
  span = float(np.abs(out_cont[:, None, :].astype(np.float64) -
                      x[None, :, :]).max())
  _report(f'{tag} dist vs fp64',
          float(np.abs(dist - o.dist.numpy()).max()), EPS * span)
  var = got.var_ws.cpu().double()
  _report(f'{tag} quad', float((var[:, T] - o.quad).abs().max()),
          sc.TOL_FP32)
  parts = var[:, :T]
  b2_err = (var[:, T] - parts.sum(1)).abs()
  b2_tol = T * EPS * parts.abs().sum(1)
  worst = int(torch.argmax(b2_err - b2_tol))
  _report(f'{tag} B2 reduce of {T} tiles', float(b2_err[worst]),
          float(b2_tol[worst]))
  assert bool((b2_err <= b2_tol).all()), tag   # NaN partials fail here

  # Phase C: every visited row has the oracle's kind.
  pool, rewards, perts = (_np(got.pool_cont), _np(got.rewards),
                          _np(got.perts))
  kinds = sw.observed_kinds(case, rewards, perts)
  assert kinds == o.kinds, (tag, kinds, o.kinds)
  cfg = oracle.Config()
  score = o.score.numpy()
  penalised = o.penalised.numpy()
  worst_reward = 0.0
  for i, kind in enumerate(kinds):
    me = start + i
    if kind == 'improved':
      assert np.array_equal(pool[me], out_cont[i]), (tag, i)
      assert perts[me] == case.perts[me]
      tol_i = sc.TOL_PENALTY if penalised[i] else sc.acq_tolerance(code)
      err_i = abs(float(rewards[me]) - float(score[i]))
      assert err_i <= tol_i, (tag, i, err_i, tol_i)
      worst_reward = max(worst_reward, err_i / tol_i)
    elif kind == 'penalised':
      assert np.array_equal(pool[me], case.pool_cont[me]), (tag, i)
      assert rewards[me] == case.rewards[me]
      assert perts[me] == F32(case.perts[me] * F32(cfg.penalize_factor))
    else:
      want = oracle.uniform(case.seed_update,
                            case.it_start ^ oracle.TAG_REFILL_CONT,
                            me * dc + np.arange(dc), F32)
      assert np.array_equal(pool[me], want), (tag, i)
      assert np.isneginf(rewards[me])
      assert perts[me] == F32(cfg.perturbation)
  print(f'OBSERVED {tag} accepted rewards: worst err/bound '
        f'{worst_reward:.3e} (bound 1)')
  for i, role in enumerate(case.roles):
    if role == 'best':                     # exempt from the restart
      assert kinds[i] == 'penalised'
      assert perts[start + i] < F32(cfg.perturbation_lower_bound)
  # The oracle's post-state: everything bitwise but the accepted rewards.
  assert np.array_equal(pool, o.pool), tag
  assert np.array_equal(perts, o.perts), tag
  accepted = np.zeros(case.pool, dtype=bool)
  accepted[start:start + batch] = [k == 'improved' for k in kinds]
  assert np.array_equal(rewards[~accepted], o.rewards[~accepted]), tag
  outside = np.ones(case.pool, dtype=bool)
  outside[start:start + batch] = False
  assert np.array_equal(pool[outside], case.pool_cont[outside])
  assert np.array_equal(rewards[outside], case.rewards[outside])
  assert np.array_equal(perts[outside], case.perts[outside])

  # Scalars.
  best = float(got.best.cpu()[0])
  top = int(np.argmax(score))
  tol_b = sc.TOL_PENALTY if penalised[top] else sc.acq_tolerance(code)
  want_best = max(float(case.best), float(score[top]))
  assert abs(best - want_best) <= tol_b, (tag, best, want_best)
  if float(score[top]) > float(case.best) + tol_b:     # a new best
    assert got.best.cpu()[0].numpy() == rewards[np.isfinite(rewards)].max()
  else:
    assert got.best.cpu()[0].numpy() == case.best
  assert got.iter_t[:2].tolist() == [case.it_start + 1, case.it_start]
  return got, o


@pytest.mark.parametrize('case_id,acq', ONE_ITERATION,
                         ids=[f'{c}-{a}' for c, a in ONE_ITERATION])
def test_one_iteration_against_fp64(ext, case_id, acq):
  case = sw.case_by_id(case_id)
  got, o = _check_iteration(ext, case, acq)
  if case_id == 'base-newbest':
    assert float(got.best.cpu()[0]) > float(case.best)
    assert set(o.kinds) == {'improved'}
  elif case.batch >= sw.FULL_ROLES_BATCH:
    assert set(o.kinds) == {'improved', 'penalised', 'dead'}


# -- (b) trust region -------------------------------------------------------------


@pytest.mark.parametrize('tr_radius', [sc.TR_RADIUS, 0.0, 0.6])
@pytest.mark.parametrize('name', sw.TR_CASES)
def test_trust_region_settings(ext, name, tr_radius):
  """0 < radius <= 0.5 penalises the far candidates with -1e4 - dist; 0 and
  0.6 both mean "no penalty". A score is seen through the reward of an
  accepted row: the low rows accept a penalised candidate too."""
  case = sw.sweep_case(name, 'tr')
  got, o = _check_iteration(ext, case, 'ucb', tr_radius)
  rewards = _np(got.rewards)[case.start:case.start + case.batch]
  improved = np.array([k == 'improved' for k in o.kinds])
  dist = o.dist.numpy()
  near = improved & (dist <= sc.TR_NEAR)
  far = improved & (dist >= sc.TR_FAR)
  assert near.sum() >= 2 and far.sum() >= 2, (near.sum(), far.sum())
  plain = sc.acquisition(0, o.mean, o.sd, sc.COEF, sw.BEST_VALUE).numpy()
  tol = sc.acq_tolerance(0)
  assert float(np.abs(rewards[near] - plain[near]).max()) <= tol
  if tr_radius == sc.TR_RADIUS:
    err = float(np.abs(rewards[far] - (-1e4 - dist[far])).max())
    _report(f'{case.name} penalised rewards', err, sc.TOL_PENALTY)
  else:
    assert not bool(o.penalised.any())
    assert float(np.abs(rewards[far] - plain[far]).max()) <= tol


# -- (c) bitwise against the step kernels ------------------------------------------

MULTI_ITERATION = (
    [(case_id, 'ucb') for case_id, shape in sw.CASES.items()
     if shape[3] < 4096] +
    [(case_id, acq) for case_id in sw.ACQ_CASES for acq in ('ei', 'pi')] +
    [('base-newbest', 'ucb')])

_FULL = {}


def _full_sweep(ext, case_id, acq='ucb'):
  """(call, seconds) of the in-process sweep of a case at its full
  iteration count; computed once, shared with the grid test."""
  if (case_id, acq) not in _FULL:
    case = sw.case_by_id(case_id)
    t0 = time.perf_counter()
    got = sw.run_sweep(ext, case, case.full_iterations(), acq=acq)
    _FULL[(case_id, acq)] = (got, time.perf_counter() - t0)
  return _FULL[(case_id, acq)]


@pytest.mark.parametrize('case_id,acq', MULTI_ITERATION,
                         ids=[f'{c}-{a}' for c, a in MULTI_ITERATION])
def test_sweep_equals_step_kernels(ext, case_id, acq):
  """One eagle_sweep call of 2 n_batches + 1 iterations against the same
  iterations of eagle_suggest -> posterior_scores_chunked -> eagle_update:
  the WHOLE state is bitwise equal.

  `large-n` is excluded: at N >= 4096 the standalone scorer takes its
  row-split k-vector kernel and one SGEMM, the sweep keeps its own k-vector
  loop and the 64x64 tiles, and the two sum in different orders, so
  equality is not expected. test_one_iteration_against_fp64 carries that
  range."""
  case = sw.case_by_id(case_id)
  its = case.full_iterations()
  got, _ = _full_sweep(ext, case_id, acq)
  want = sw.compose_step_kernels(ext, case, its, acq=acq)
  assert torch.equal(got.pool_cont, want.pool_cont)
  assert torch.equal(got.rewards, want.rewards)
  assert torch.equal(got.perts, want.perts)
  assert torch.equal(got.best, want.best)
  last = case.it_start + its - 1
  assert got.iter_t[:2].tolist() == want.iter_t[:2].tolist() == [last + 1,
                                                                 last]
  assert not torch.equal(got.pool_cont.cpu(),
                         torch.from_numpy(case.pool_cont))
  if case_id != 'base-newbest':
    assert want.dead >= 1, 'no firefly was restarted in this run'


# -- (d) grid sizes: one fresh child process each ------------------------------------

_child_failed = []


@pytest.mark.parametrize('grid', sw.GRIDS)
def test_grid_override_in_child(ext, tmp_path, grid):
  """VIZIER_AMD_SWEEP_GRID = 1, 7 (below the batch size: Phases A, B2 and C
  stride) and 200 (above the launcher's cap of 128): the full final state
  equals the in-process sweep at the default grid."""
  if _child_failed:
    pytest.fail(f'child grid={_child_failed[0]} failed earlier; '
                'not starting another')
  cases = [sw.case_by_id(c) for c in sw.GRID_CASES]
  want = [_full_sweep(ext, c) for c in sw.GRID_CASES]
  # A hang guard, not a performance claim.
  limit = max(60.0, 20.0 * sum(seconds for _, seconds in want))
  env = dict(os.environ)
  env['VIZIER_AMD_SWEEP_GRID'] = str(grid)
  env['PYTHONPATH'] = os.pathsep.join(
      [_REPO, _TESTS] + [p for p in [env.get('PYTHONPATH')] if p])
  out = tmp_path / 'child.npz'
  cmd = [sys.executable, '-m', 'sweep_cases', '--out', str(out),
         '--cases', ','.join(sw.GRID_CASES), '--iterations',
         ','.join(str(c.full_iterations()) for c in cases)]
  try:
    res = subprocess.run(cmd, env=env, cwd=_REPO, capture_output=True,
                         text=True, timeout=limit)
  except subprocess.TimeoutExpired:
    _child_failed.append(grid)
    pytest.fail(f'child grid={grid} timed out after {limit:.0f} s')
  if res.returncode != 0:
    _child_failed.append(grid)
    pytest.fail(f'child grid={grid} exited {res.returncode}:\n'
                f'{res.stderr[-2000:]}')
  child = np.load(out)
  for case_id, (call, _) in zip(sw.GRID_CASES, want):
    assert int(child[f'{case_id}/grid']) == grid, case_id
    assert call.grid != grid
    for key, t in (('pool_cont', call.pool_cont), ('rewards', call.rewards),
                   ('perts', call.perts), ('best', call.best),
                   ('iter', call.iter_t[:2])):
      assert torch.equal(torch.from_numpy(child[f'{case_id}/{key}']),
                         t.cpu()), (grid, case_id, key)


# -- (e) arguments -------------------------------------------------------------------


def test_binding_rejects_bad_arguments(ext):
  """Each of these raises before any launch, and leaves the caller's
  tensors as they were."""
  case = sw.sweep_case('base')
  pool, batch, dc, n = sw.CASES['base']
  call = sw.sweep_call(case, 1)
  before = [t.clone() for t in call.state()]
  iter_before = call.iter_t.clone()
  dev = 'cuda'

  def rejected(**replace):
    with pytest.raises(RuntimeError):
      ext.eagle_sweep(*dataclasses.replace(call, **replace).args())
    torch.cuda.synchronize()
    for t, b in zip(call.state(), before):
      assert torch.equal(t, b), replace.keys()
    assert torch.equal(call.iter_t, iter_before), replace.keys()
    assert bool(torch.isnan(call.out_cont).all()), replace.keys()
    assert bool(torch.isnan(call.var_ws).all()), replace.keys()

  def f32(*shape):
    return torch.rand(*shape, dtype=torch.float32, device=dev)

  # dc = 513 would write past xq_lds[512]; dc = 0 divides by it.
  for wide in (513, 0):
    rejected(x=f32(n, wide), inv_ls=f32(wide), pool_cont=f32(pool, wide),
             out_cont=f32(batch, wide))
  # The in/out state: never copied, so never non-contiguous or converted.
  rejected(pool_cont=f32(2 * pool, dc)[::2])
  rejected(rewards=f32(2 * pool)[::2])
  rejected(perts=f32(2 * pool)[::2])
  for name in ('pool_cont', 'rewards', 'perts'):
    rejected(**{name: getattr(call, name).double()})
    rejected(**{name: getattr(call, name).cpu()})
  rejected(best=call.best.double())
  rejected(best=call.best.cpu())
  rejected(best=call.best[:0])
  rejected(iter_t=call.iter_t.int())
  rejected(iter_t=call.iter_t[:11].contiguous())
  rejected(barrier=call.barrier.cpu())
  rejected(out_cont=f32(batch * dc - 1))
  rejected(k_ws=f32(batch * n - 1))
  rejected(mu_ws=f32(batch - 1))
  rejected(dist_ws=f32(batch - 1))
  rejected(alpha=f32(n - 1))
  rejected(inv_ls=f32(dc - 1))
  rejected(M=f32(n, n - 1))
  rejected(M=f32(n - 1, n - 1))
  rejected(M=f32(n * n))
  rejected(rewards=f32(pool - 1))
  rejected(perts=f32(pool + 1))
  rejected(n_batches=3)
  rejected(pool=pool - batch)          # pool_cont no longer matches
  rejected(batch=0)
  rejected(batch=0, n_batches=0)
  rejected(iterations=-1)

  # iterations = 0 launches, changes nothing, and publishes the counters.
  ext.eagle_sweep(*dataclasses.replace(call, iterations=0).args())
  torch.cuda.synchronize()
  for t, b in zip(call.state(), before):
    assert torch.equal(t, b)
  assert call.iter_t[:2].tolist() == [case.it_start, case.it_start - 1]
  # And the unmodified call is valid.
  assert ext.eagle_sweep(*call.args()) >= 1
  torch.cuda.synchronize()
  assert call.iter_t[:2].tolist() == [case.it_start + 1, case.it_start]
  assert not torch.equal(call.pool_cont, before[0])


# -- (f) the optimizer's glue ----------------------------------------------------------

_PROBLEM = {}


def _posterior(n=130, d=3, seed=0):
  if not _PROBLEM:
    from vizier_amd._src.gp import gp_model
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, d, generator=g).cuda()
    y = (-((x - 0.4) ** 2).sum(-1) +
         0.01 * torch.randn(n, generator=g).cuda())
    _PROBLEM['post'] = gp_model.train_gp(x, y, num_restarts=1, max_iters=5)
  return _PROBLEM['post'], d


def _optimize(scoring, d, *, force_graph, evals=1500, seed=7):
  from vizier_amd._src.algorithms.optimizers.eagle import (
      EagleStrategyConfig)
  from vizier_amd._src.algorithms.optimizers.vectorized import (
      VectorizedOptimizerFactory)
  factory = VectorizedOptimizerFactory(
      eagle_config=EagleStrategyConfig(), max_evaluations=evals,
      suggestion_batch_size=25)
  opt = factory(n_continuous=d, categorical_sizes=[], n_parallel=1,
                seed=seed, device='cuda', dtype=torch.float32)
  if force_graph:
    opt._megakernel_applicable = lambda score_fn: False

  def score_fn(batch):
    return scoring(batch.continuous[:, 0, :])
  score_fn.scoring = scoring
  score_fn.codec_identity = True
  return opt, opt.optimize(score_fn, count=opt.strategy.pool_size)


@pytest.mark.parametrize('acq,trust_region', [
    ('ucb', True), ('ei', True), ('pi', False), ('lcb', True)])
def test_optimizer_paths_agree_for_every_acquisition(ext, monkeypatch, acq,
                                                     trust_region):
  """The megakernel path and the hipGraph path of the optimizer return the
  same WHOLE final pool, bitwise: catches a transposed positional argument
  of _optimize_megakernel (coef and best differ for every variant)."""
  from vizier_amd._src.gp import acquisitions as acq_lib
  monkeypatch.setenv('VIZIER_AMD_MEGAKERNEL', '1')
  post, d = _posterior()
  acquisition = {'ucb': acq_lib.UCB(coefficient=1.8),
                 'lcb': acq_lib.LCB(coefficient=1.8),
                 'ei': acq_lib.EI(best_value=-0.2),
                 'pi': acq_lib.PI(best_value=-0.2)}[acq]
  tr = None
  if trust_region:
    tr = acq_lib.TrustRegion(
        post.x, torch.zeros(d, dtype=torch.bool, device='cuda'))
  scoring = acq_lib.ScoringFunction(post, acquisition, tr)
  assert scoring._coef != scoring._best
  opt_g, res_g = _optimize(scoring, d, force_graph=True)
  assert opt_g.last_used_graph and not opt_g.last_used_megakernel, \
      opt_g.last_graph_error
  opt_m, res_m = _optimize(scoring, d, force_graph=False)
  assert opt_m.last_used_megakernel, opt_m.last_graph_error
  assert res_m.rewards.numel() == opt_m.strategy.pool_size
  assert torch.equal(res_m.rewards, res_g.rewards)
  assert torch.equal(res_m.features.continuous, res_g.features.continuous)
