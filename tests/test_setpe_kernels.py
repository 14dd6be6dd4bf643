"""The fused set-PE scorer (setpe_score.hip) against fp64 references.

  setpe_scores_from_cov  setpe_logdet_kernel: jitter, q x q Cholesky in one
                         wave, logdet or -inf, promising-region penalty,
                         per-member trust region
  setpe_set_scores       explore (mean, sd) + joint covariance and distances
                         under the completed + pending posterior + the tail
  set_pe_scorer='hip'    the designer's set sweep through the hipGraph path

Operands and references: tests/setpe_cases.py (two real fp64 GPs rounded once
to fp32; the reference is the torch closure of _set_pe_score_fn in float64 on
the CPU).

Bounds.
  tail   hand-made inputs with closed-form fp64 values, bound
         q 2^-22 (max(1, max|log pivot|) + sum|penalty terms| +
         sum|trust-region terms|). Bad covariances score exactly -inf, and a
         good set scores the same bit for bit with or without bad neighbours.
  end to end on the dense shapes: MEASURED margin. The same fp32 operands go
         through the fp32 torch closure on the GPU (the code this scorer
         replaces); its largest error against fp64 over the whole shape
         family, times 4 (only the summation order and the logdet form
         differ), floored at 16 q 2^-24 max(1, |score_ref|), is the
         tolerance.

`pytest -rA` prints every figure (OBSERVED lines). Largest errors observed on
the MI355X next to the bound they were held to:
  tail    diagonal q = 1 / 2 / 16: 8.3e-07 / 7.8e-07 / 2.2e-06 (bounds
          1.5e-06 / 2.9e-06 / 2.6e-05); 2 x 2: 6.3e-08 (6.6e-07); penalty
          8.9e-07 (1.4e-05); trust region 2.0e-04 (9.5e-03), exactly 0 with
          the region off or dist = None; all terms 7.8e-04 (9.6e-03); mixed
          batch 4.3e-04 (4.8e-03)
  duplicate members  -inf; the other sets -40.5 .. -14.7
  e2e dense   fp32 torch 3.2e-03 (margin 1.3e-02), kernel 3.3e-03; per shape
          kernel / torch 5.1e-05 / 4.3e-04, 1.2e-04 / 3.7e-05, 3.0e-04 /
          3.0e-04, 3.3e-03 / 3.2e-03, 2.5e-03 / 2.1e-03: both carry the fp32
          rounding of the covariance through 1 / lambda_min
  trust region  6.6e-03 (bound 5.3e-01; 118 of 200 members outside, scores
          about -1e5), 1.1e-02 (2.3e+00; 391 of 528 outside)
  designer    hip scorer against the torch closure on the fitted designer:
          relative 1.0e-05
"""

import numpy as np
import pytest
import torch

import setpe_cases as pc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
INF = float('inf')


def _ids(shapes):
  return ['x'.join(str(v) for v in s) for s in shapes]


@pytest.fixture(scope='module')
def ext():
  from vizier_amd._src.ops import dispatch
  return dispatch.require_ext()  # Fails loudly if the .so is missing.


class Ops:
  """A case's tensors on the GPU."""

  def __init__(self, case, onehot=None):
    self.case = case
    self.xs = case.xs.to(DEV)
    self.x = case.explore.x.to(DEV)
    self.alpha = case.explore.alpha.to(DEV)
    self.kinv = case.explore.kinv.to(DEV)
    self.x_all = case.var.x.to(DEV)
    self.kinv_all = case.var.kinv.to(DEV)
    self.ls = case.explore.ls.to(DEV)
    self.onehot = torch.tensor(onehot if onehot is not None
                               else [0] * case.d, dtype=torch.uint8,
                               device=DEV)

  def scores(self, ext, tr_radius=0.0, xs=None):
    return ext.setpe_set_scores(
        self.xs if xs is None else xs, self.x, self.alpha, self.kinv,
        pc.sc.MEAN_C, self.x_all, self.kinv_all, self.ls, pc.sc.AMP,
        self.onehot, self.case.threshold, pc.EXPLORE_COEF, pc.PENALTY_COEF,
        tr_radius)


@pytest.fixture(scope='module')
def dense_ops():
  return {shape: Ops(pc.dense_case(*shape)) for shape in pc.DENSE_SHAPES}


# -- 1. the tail on hand-made inputs ------------------------------------------


def test_tail_handmade_values(ext):
  for tail in pc.handmade_tails():
    got = ext.setpe_scores_from_cov(*tail.args(DEV)).cpu().double()
    assert got.shape == tail.want.shape
    err = (got - tail.want).abs()
    print(f'OBSERVED tail {tail.name}: {float(err.max()):.3e} (bound '
          f'{float(tail.bound[err.argmax()]):.3e}), '
          f'{float((err / tail.bound).max()):.3f} of the bound')
    assert bool((err <= tail.bound).all()), tail.name


def test_tail_jitter_is_added_to_the_diagonal(ext):
  # cov = 0 with jitter j: logdet = q log(j), and fl(d + j) for a diagonal.
  z = torch.zeros(1, 3, device=DEV)
  got = ext.setpe_scores_from_cov(torch.zeros(1, 3, 3, device=DEV), z, z,
                                  None, 1e-6, 0.0, 0.5, 10.0, 0.0)
  log_j = float(np.log(float(np.float32(1e-6))))
  assert abs(float(got[0]) - 3.0 * log_j) <= 3 * 2.0 ** -22 * abs(log_j)
  # d + 0.25 is exact in fp32 for these values.
  d = torch.tensor([0.5, 2.0, 1.0])
  got = ext.setpe_scores_from_cov(torch.diag(d).view(1, 3, 3).to(DEV), z, z,
                                  None, 0.25, 0.0, 0.5, 10.0, 0.0)
  want = float((d.double() + 0.25).log().sum())
  assert abs(float(got[0]) - want) <= 3 * 2.0 ** -22


# -- 2. the failure path --------------------------------------------------------


def _zeros(b, q):
  return torch.zeros(b, q, device=DEV)


def test_bad_covariances_score_exactly_minus_infinity(ext):
  cov = torch.tensor(pc.BAD_COVS, device=DEV)
  z = _zeros(len(pc.BAD_COVS), 2)
  got = ext.setpe_scores_from_cov(cov, z, z, None, 0.0, 0.0, 0.5, 10.0, 0.0)
  assert got.cpu().tolist() == [-INF] * len(pc.BAD_COVS)
  # ... with a penalty and a trust-region term on top.
  mean = torch.full_like(z, -1.0)
  dist = torch.full_like(z, 0.4)
  got = ext.setpe_scores_from_cov(cov, mean, z, dist, 0.0, 0.0, 0.5, 10.0,
                                  0.3)
  assert got.cpu().tolist() == [-INF] * len(pc.BAD_COVS)
  # q = 16: a bad LAST pivot, and NaN in the last row only.
  for bad in (-1.0, pc.NAN):
    big = torch.eye(16).view(1, 16, 16).clone()
    big[0, 15, 15] = bad
    z16 = _zeros(1, 16)
    got = ext.setpe_scores_from_cov(big.to(DEV), z16, z16, None, 0.0, 0.0,
                                    0.5, 10.0, 0.0)
    assert float(got[0]) == -INF


def test_bad_sets_do_not_leak_into_good_ones(ext):
  # Five sets in two workgroups of four waves: bad and good interleaved.
  covs = [pc.GOOD_COVS[0], pc.BAD_COVS[0], pc.GOOD_COVS[1], pc.BAD_COVS[2],
          pc.GOOD_COVS[2]]
  cov = torch.tensor(covs, device=DEV)
  g = torch.Generator().manual_seed(8)
  mean = (torch.rand(5, 2, generator=g) - 0.5).to(DEV)
  sd = torch.rand(5, 2, generator=g).to(DEV)
  dist = torch.rand(5, 2, generator=g).to(DEV)
  args = (1e-6, 0.1, 0.5, 10.0, 0.3)
  got = ext.setpe_scores_from_cov(cov, mean, sd, dist, *args).cpu()
  assert [bool(torch.isfinite(v)) for v in got] == [True, False, True,
                                                    False, True]
  assert got[1] == -INF and got[3] == -INF
  want, logdet, pen, tr, _ = pc.tail_reference(
      cov.cpu().double(), mean.cpu().double(), sd.cpu().double(),
      dist.cpu().double(), float(np.float32(1e-6)), float(np.float32(0.1)),
      0.5, 10.0, float(np.float32(0.3)))
  good = [0, 2, 4]
  err = (got[good].double() - want[good]).abs()
  # As the hand-made tails; |logdet| >= max|log pivot| for these sets (no
  # two pivots on opposite sides of 1).
  bound = 2 * 2.0 ** -22 * (logdet[good].abs().clamp_min(1.0) +
                            pen[good].abs() + tr[good].abs())
  print(f'OBSERVED mixed batch: {float(err.max()):.3e} (bound '
        f'{float(bound.min()):.3e})')
  assert bool((err <= bound).all())
  # A good set scores the same, bit for bit, alone.
  alone = ext.setpe_scores_from_cov(cov[good], mean[good], sd[good],
                                    dist[good], *args).cpu()
  assert torch.equal(alone, got[good])


# -- 3. duplicate members ---------------------------------------------------------


def test_duplicate_members_rank_below_every_other_set(ext, dense_ops):
  ops = dense_ops[25, 8, 255, 2, 20]
  xs = ops.xs.clone()
  xs[7, 5] = xs[7, 2]                 # two identical candidates in set 7
  got = ops.scores(ext, xs=xs).cpu()
  others = torch.cat([got[:7], got[8:]])
  assert bool(torch.isfinite(others).all())
  print(f'OBSERVED duplicate set: {float(got[7])}, others '
        f'{float(others.min()):.3f} .. {float(others.max()):.3f}')
  assert float(got[7]) == -INF or bool(torch.isfinite(got[7]))
  assert float(got[7]) < float(others.min())
  # The other sets do not notice.
  base = ops.scores(ext).cpu()
  assert torch.equal(others, torch.cat([base[:7], base[8:]]))


# -- 4. dense, end to end, measured margin ------------------------------------------


@pytest.fixture(scope='module')
def family(ext, dense_ops):
  """Kernel and fp32-torch score errors against fp64 over the shape family."""
  rows = {}
  for shape in pc.DENSE_SHAPES:
    case = pc.dense_case(*shape)
    ref = pc.dense_reference(*shape)
    got = dense_ops[shape].scores(ext).cpu().double()
    emu = pc.reference(case, torch.float32, DEV).scores.cpu().double()
    rows[shape] = dict(kernel=(got - ref.scores).abs(),
                       torch=(emu - ref.scores).abs(),
                       floor=pc.score_floor(case.q, ref.scores))
  return rows


def test_dense_scores_within_measured_margin(family):
  torch_max = max(float(r['torch'].max()) for r in family.values())
  kernel_max = max(float(r['kernel'].max()) for r in family.values())
  print(f'OBSERVED e2e: fp32 torch max error {torch_max:.3e} (margin 4x = '
        f'{4 * torch_max:.3e}), kernel max error {kernel_max:.3e}')
  for shape, r in family.items():
    print(f'  e2e {shape}: kernel {float(r["kernel"].max()):.3e}, torch '
          f'{float(r["torch"].max()):.3e}, floor '
          f'{float(r["floor"].min()):.3e}')
  for shape, r in family.items():
    tol = r['floor'].clamp_min(4.0 * torch_max)
    assert bool((r['kernel'] <= tol).all()), shape


@pytest.mark.parametrize('shape', [pc.DENSE_SHAPES[2], pc.DENSE_SHAPES[3]],
                         ids=_ids([pc.DENSE_SHAPES[2], pc.DENSE_SHAPES[3]]))
def test_dense_scores_with_a_trust_region(ext, family, dense_ops, shape):
  case, ref = pc.dense_case(*shape), pc.dense_reference(*shape)
  radius = pc.split_radius(ref.dist)
  assert 0.0 < radius <= 0.5
  want = pc.reference(case, region=pc.trust_region(case, radius))
  assert bool((want.tr < 0).any())
  got = dense_ops[shape].scores(ext, tr_radius=radius).cpu().double()
  torch_max = max(float(r['torch'].max()) for r in family.values())
  tol = pc.score_floor(case.q, want.scores).clamp_min(4.0 * torch_max)
  err = (got - want.scores).abs()
  print(f'OBSERVED trust region {shape}: radius {radius:.4f}, '
        f'{int((ref.dist > radius).sum())} of {ref.dist.numel()} members '
        f'outside, error {float(err.max()):.3e} (bound '
        f'{float(tol[err.argmax()]):.3e})')
  assert bool((err <= tol).all())
  # Radius 0.6: the region is off.
  assert torch.equal(dense_ops[shape].scores(ext, tr_radius=0.6),
                     dense_ops[shape].scores(ext))


def test_trust_region_mask_excludes_columns(ext):
  # A masked column must not count: move every candidate far away along it.
  shape = pc.DENSE_SHAPES[1]                      # d = 3
  case = pc.dense_case(*shape)
  masked = Ops(case, onehot=[0, 1, 0])
  xs = masked.xs.clone()
  xs[:, :, 1] = 5.0
  dist = pc.sc.min_linf_dist(case.xs.double().reshape(-1, case.d),
                             case.var.x.double(), [0, 1, 0])
  radius = float(np.float32(float(dist.max()) * 1.01))
  assert radius <= 0.5
  # Inside on the unmasked columns: no trust-region term, although column 1
  # is 4 away; the kernel value must stay finite and un-penalised.
  got = masked.scores(ext, tr_radius=radius, xs=xs).cpu()
  assert bool((got > -1e3).all())
  assert bool((Ops(case).scores(ext, tr_radius=radius, xs=xs).cpu()
               < -1e4).all())


# -- 5. determinism -----------------------------------------------------------------


def test_set_scores_are_deterministic(ext, dense_ops):
  for shape in (pc.DENSE_SHAPES[2], pc.DENSE_SHAPES[3]):
    ops = dense_ops[shape]
    assert torch.equal(ops.scores(ext), ops.scores(ext))
    assert torch.equal(ops.scores(ext, tr_radius=0.3),
                       ops.scores(ext, tr_radius=0.3))


# -- 6. limits ------------------------------------------------------------------------


def _small_args(q=2, d=3, n=8, p=2, **over):
  z = lambda *shape: torch.zeros(*shape, device=DEV)
  args = dict(
      xs=torch.rand(2, q, d, device=DEV), post_x=torch.rand(n, d, device=DEV),
      post_alpha=z(n), post_kinv=z(n, n), post_mean_c=0.0,
      all_x=torch.rand(n + p, d, device=DEV), all_kinv=z(n + p, n + p),
      lengthscales=torch.ones(d, device=DEV), amplitude=1.0,
      onehot=torch.zeros(d, dtype=torch.uint8, device=DEV), threshold=0.0,
      explore_coef=0.5, penalty_coef=10.0, tr_radius=0.0)
  args.update(over)
  return tuple(args.values())


def test_limits_raise(ext):
  z = lambda *shape: torch.zeros(*shape, device=DEV)
  assert ext.setpe_set_scores(*_small_args(q=16)).shape == (2,)
  assert ext.setpe_set_scores(*_small_args(d=512)).shape == (2,)
  with pytest.raises(RuntimeError, match='q <= 16'):
    ext.setpe_set_scores(*_small_args(q=17))
  with pytest.raises(RuntimeError, match='D <= 512'):
    ext.setpe_set_scores(*_small_args(d=513))
  with pytest.raises(RuntimeError, match='all_kinv'):
    ext.setpe_set_scores(*_small_args(all_kinv=z(8, 8)))
  with pytest.raises(RuntimeError, match='all_x'):
    ext.setpe_set_scores(*_small_args(all_x=z(10, 4)))
  with pytest.raises(RuntimeError, match='kinv'):
    ext.setpe_set_scores(*_small_args(post_kinv=z(7, 7)))
  with pytest.raises(RuntimeError, match='alpha'):
    ext.setpe_set_scores(*_small_args(post_alpha=z(9)))
  with pytest.raises(RuntimeError, match='lengthscales'):
    ext.setpe_set_scores(*_small_args(lengthscales=z(4)))
  with pytest.raises(RuntimeError, match='fp32'):
    ext.setpe_set_scores(*_small_args(
        xs=torch.rand(2, 2, 3, device=DEV, dtype=torch.float64)))
  with pytest.raises(RuntimeError, match='B, q, D'):
    ext.setpe_set_scores(*_small_args(xs=torch.rand(4, 3, device=DEV)))
  tail = (0.0, 0.0, 0.5, 10.0, 0.0)
  with pytest.raises(RuntimeError, match='q <= 16'):
    ext.setpe_scores_from_cov(z(2, 17, 17), z(2, 17), z(2, 17), None, *tail)
  with pytest.raises(RuntimeError, match='cov'):
    ext.setpe_scores_from_cov(z(2, 2, 3), z(2, 2), z(2, 2), None, *tail)
  with pytest.raises(RuntimeError, match='mean'):
    ext.setpe_scores_from_cov(z(2, 2, 2), z(2, 3), z(2, 2), None, *tail)
  with pytest.raises(RuntimeError, match='sd'):
    ext.setpe_scores_from_cov(z(2, 2, 2), z(2, 2), z(3, 2), None, *tail)
  with pytest.raises(RuntimeError, match='dist'):
    ext.setpe_scores_from_cov(z(2, 2, 2), z(2, 2), z(2, 2), z(5), *tail)
  with pytest.raises(RuntimeError, match='at least one'):
    ext.setpe_scores_from_cov(z(0, 2, 2), z(0, 2), z(0, 2), None, *tail)
  with pytest.raises(RuntimeError, match='fp32'):
    ext.setpe_scores_from_cov(z(2, 2, 2).double(), z(2, 2), z(2, 2), None,
                              *tail)


# -- 7. the designer: capture and the suggest loop -------------------------------------


def _problem():
  from vizier_amd import pyvizier as vz
  problem = vz.ProblemStatement()
  for i in range(4):
    problem.search_space.root.add_float_param(f'x{i}', 0.0, 1.0)
  problem.metric_information.append(vz.MetricInformation(
      name='obj', goal=vz.ObjectiveMetricGoal.MAXIMIZE))
  return problem


def _trial(uid, rng, complete=True):
  from vizier_amd import pyvizier as vz
  params = {f'x{i}': float(rng.uniform()) for i in range(4)}
  t = vz.Trial(params, id=uid)
  if complete:
    t.complete(vz.Measurement(
        metrics={'obj': -sum((v - 0.5) ** 2 for v in params.values())}))
  return t


def _fitted_designer(n_trials=24, n_pending=2, **kw):
  """(designer, x_all): fitted on n_trials, n_pending active trials."""
  from vizier_amd._src.algorithms.core.abstractions import (
      ActiveTrials,
      CompletedTrials,
  )
  from vizier_amd._src.algorithms.designers.gp_ucb_pe import (
      UCBPEConfig,
      VizierGPUCBPEBandit,
  )
  d = VizierGPUCBPEBandit(_problem(), UCBPEConfig(
      optimize_set_acquisition_for_exploration=True, ard_restarts=1,
      ard_max_iters=10, device='cuda', **kw), seed=1)
  rng = np.random.default_rng(0)
  done = [_trial(uid, rng) for uid in range(1, n_trials + 1)]
  active = [_trial(n_trials + 1 + i, rng, complete=False)
            for i in range(n_pending)]
  d.update(CompletedTrials(done), ActiveTrials(active))
  d._fit()
  pending = torch.as_tensor(d._converter.to_features(active),
                            dtype=d._config.dtype, device=d._device)
  return d, torch.cat([d._posterior.x, pending], dim=0)


def _sweep(d, score_fn, q, x_all):
  """optimizer.optimize(count=1) built the way _optimize_set builds it."""
  from vizier_amd._src.algorithms.optimizers.eagle import EagleStrategyConfig
  from vizier_amd._src.algorithms.optimizers.vectorized import (
      VectorizedOptimizerFactory,
  )
  cfg = d._config
  optimizer = VectorizedOptimizerFactory(
      eagle_config=EagleStrategyConfig(),
      max_evaluations=cfg.max_evaluations,
      suggestion_batch_size=cfg.suggestion_batch_size)(
          n_continuous=d._codec.n_continuous,
          categorical_sizes=d._codec.categorical_sizes, n_parallel=q,
          seed=d._seed + len(d._completed) + x_all.shape[0],
          device=d._device, dtype=cfg.dtype)
  return optimizer, optimizer.optimize(score_fn, count=1)


def test_hip_scorer_sweep_is_captured_and_matches_eager(ext):
  d, x_all = _fitted_designer(set_pe_scorer='hip', max_evaluations=2000)
  score_fn = d._set_pe_score_fn(x_all, 3)
  assert score_fn.graph_safe is True
  captured, got = _sweep(d, score_fn, 3, x_all)
  assert captured.last_used_graph is True
  assert captured.last_graph_error is None

  def eager_fn(batch):
    return score_fn(batch)
  eager_fn.graph_safe = False          # forces the eager loop
  eager, want = _sweep(d, eager_fn, 3, x_all)
  assert eager.last_used_graph is False
  # count = 1: the final-pool selection of the captured sweep is exact.
  assert torch.equal(got.rewards, want.rewards)
  assert torch.equal(got.features.continuous, want.features.continuous)
  assert got.features.continuous.shape == (1, 3, 4)
  assert bool(torch.isfinite(got.rewards).all())
  # The process is not left in capture mode.
  assert float(torch.ones(8, device=DEV).sum()) == 8.0
  assert not torch.cuda.is_current_stream_capturing()


def test_hip_scorer_agrees_with_the_torch_closure(ext):
  # Same fitted designer state, both scorers, one random batch of sets.
  from vizier_amd._src.algorithms.optimizers.eagle import CandidateBatch
  d, x_all = _fitted_designer(set_pe_scorer='hip', max_evaluations=200)
  hip_fn = d._set_pe_score_fn(x_all, 3)
  d._config.set_pe_scorer = 'torch'
  torch_fn = d._set_pe_score_fn(x_all, 3)
  assert hip_fn.graph_safe is True and torch_fn.graph_safe is False
  g = torch.Generator().manual_seed(3)
  batch = CandidateBatch(
      torch.rand(25, 3, 4, generator=g).to(DEV),
      torch.zeros(25, 3, 0, dtype=torch.long, device=DEV))
  got, want = hip_fn(batch).cpu(), torch_fn(batch).cpu()
  fin = torch.isfinite(want)
  assert bool(fin.any())
  err = (got[fin] - want[fin]).abs() / want[fin].abs().clamp_min(1.0)
  print(f'OBSERVED designer hip vs torch closure: relative '
        f'{float(err.max()):.3e}')
  # A wiring check, not an accuracy one (that is the dense test): a wrong
  # posterior, threshold or coefficient moves a score by O(1) or more, the
  # fp32 rounding of either side by orders of magnitude less.
  assert float(err.max()) <= 1e-2


def test_default_scorer_is_still_not_offered_for_capture(ext):
  d, x_all = _fitted_designer(max_evaluations=200)
  assert d._set_pe_score_fn(x_all, 3).graph_safe is False
  # More members than the kernels take: the torch closure.
  d, x_all = _fitted_designer(set_pe_scorer='hip', max_evaluations=200)
  assert d._set_pe_score_fn(x_all, 17).graph_safe is False
  assert d._set_pe_score_fn(x_all, 16).graph_safe is True


def test_hip_scorer_with_linear_kernel_stays_on_torch(ext):
  d, x_all = _fitted_designer(set_pe_scorer='hip', max_evaluations=200,
                              mixes_linear_kernel=True)
  assert d._set_pe_score_fn(x_all, 3).graph_safe is False


def test_hip_scorer_suggest_loop(ext):
  from vizier_amd import pyvizier as vz
  from vizier_amd._src.algorithms.core.abstractions import (
      ActiveTrials,
      CompletedTrials,
  )
  from vizier_amd._src.algorithms.designers.gp_ucb_pe import (
      UCBPEConfig,
      VizierGPUCBPEBandit,
  )
  d = VizierGPUCBPEBandit(_problem(), UCBPEConfig(
      optimize_set_acquisition_for_exploration=True, set_pe_scorer='hip',
      max_evaluations=1500, ard_restarts=1, ard_max_iters=10,
      device='cuda'), seed=1)
  rng = np.random.default_rng(0)
  d.update(CompletedTrials([_trial(uid, rng) for uid in range(1, 9)]),
           ActiveTrials())
  uid = 8
  for _ in range(3):
    batch = d.suggest(4)
    assert len(batch) == 4
    labels = [s.metadata.ns('gp_ucb_pe')['acquisition'] for s in batch]
    assert labels == ['ucb', 'set_pe', 'set_pe', 'set_pe']
    assert d._last_set_optimizer.last_used_graph is True
    assert d._last_set_optimizer.last_graph_error is None
    trials = []
    for s in batch:
      uid += 1
      x = np.array([s.parameters.get_value(f'x{i}') for i in range(4)])
      assert bool(((x >= 0.0) & (x <= 1.0)).all())
      t = s.to_trial(uid)
      t.complete(vz.Measurement(
          metrics={'obj': float(-((x - 0.5) ** 2).sum())}))
      trials.append(t)
    d.update(CompletedTrials(trials), ActiveTrials())
