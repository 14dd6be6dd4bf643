"""The fused qEI set scorer (qei_score.hip) against fp64 references.

  qei_joint_mean_cov   ps_kvec + one SGEMM against K^-1 + qei_cov_kernel
  qei_scores_from_cov  qei_mc_kernel: jitter, q x q Cholesky in one wave,
                       diagonal fallback, Monte-Carlo max-improvement
  qei_set_scores       both, plus the trust region by member 0
  qei_scorer='hip'     the designer's sweep through the hipGraph path

Operands and references: tests/qei_cases.py (a real fp64 GP rounded once to
fp32; the reference is posterior_batched_cov + qei_mc_scores in float64 on
the CPU).

Bounds.
  joint  DERIVED per entry from the reference's own operands
         (qei_cases.joint_bounds, u = 2^-24): 8 N u |k_r|^T |Kinv| |k_c| for
         the two chained N-term sums, the k-vector's own rounding
         4 (D + 16) 2^-23 amp^2 per element through |Kinv| and alpha, and
         2^-23 |mean_c|. cov must be EXACTLY symmetric, dist within an fp32
         ulp of scorer_cases.min_linf_dist of member 0.
  spikes alpha = e_i, Kinv = c (e_i e_j^T + e_j e_i^T): the mean and the
         quadratic form read single k entries, relative tolerance
         sc.TOL_SPIKE_REL.
  mc     hand-made covariances with closed-form fp64 values, bound
         q 2^-22 max|y| (diagonal) or qei_cases.mc_floor.
  mc / end to end on the dense shapes: MEASURED margin. The same fp32
         inputs go through the fp32 torch code on the GPU (the code this
         scorer replaces); its largest error against fp64 over the whole
         shape family, times 4 (only the summation order differs), floored
         at 16 q 2^-24 max(|mean| + |L||eps|), is the tolerance.

`pytest -rA` prints every figure. Largest errors observed on the MI355X next
to the bound they were held to (OBSERVED lines):
  joint   mean 5.6e-06 .. 3.0e-05 (smallest bound 1.1e-02), cov 1.7e-06 ..
          7.6e-05 (smallest bound 4.7e-02)
  spikes  mean 2.1e-07, quad 5.1e-07 (bound 1e-05)
  mc      diagonal q = 1: 0.036 of the bound; covariance statistic: kernel
          0.4862659, fp64 0.4862659 (L^T eps would give 0.5735017);
          fallback 2.6e-08 (bound 3.8e-06), mixed batch 3.0e-08 (9.4e-06)
  mc dense    fp32 torch 1.8e-07 .. 2.7e-07 over two runs (margin 7.2e-07 ..
          1.1e-06), kernel 2.1e-07 .. 2.6e-07; every case was held to its
          floor (4.0e-07 .. 4.5e-05) or the margin, whichever is larger
  e2e dense   fp32 torch 3.1e-04 (margin 1.2e-03), kernel 2.4e-04
  trust region  inside 1.7e-05 (bound 1.2e-03), penalised 2.0e-04 (2e-03)
"""

import numpy as np
import pytest
import torch

import qei_cases as qc
import scorer_cases as sc

pytestmark = pytest.mark.gpu

DEV = 'cuda'


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
    self.x = case.x.to(DEV)
    self.xs = case.xs.to(DEV)
    self.ls = case.ls.to(DEV)
    self.alpha = case.alpha.to(DEV)
    self.kinv = case.kinv.to(DEV)
    self.eps = case.eps.to(DEV)
    if onehot is None:
      onehot = [0] * case.d
    self.onehot = torch.tensor(onehot, dtype=torch.uint8, device=DEV)

  def joint(self, ext, alpha=None, kinv=None):
    return ext.qei_joint_mean_cov(
        self.xs, self.x, self.ls, sc.AMP, sc.MEAN_C,
        self.alpha if alpha is None else alpha,
        self.kinv if kinv is None else kinv, self.onehot)

  def scores(self, ext, s, tr_radius=0.0):
    return ext.qei_set_scores(
        self.xs, self.x, self.ls, sc.AMP, sc.MEAN_C, self.alpha, self.kinv,
        self.onehot, self.eps[:s].contiguous(), self.case.best, tr_radius)


@pytest.fixture(scope='module')
def dense_ops():
  return {shape: Ops(qc.dense_case(*shape)) for shape in qc.DENSE_SHAPES}


# -- 1. joint mean / covariance -----------------------------------------------


@pytest.mark.parametrize('shape', qc.DENSE_SHAPES, ids=_ids(qc.DENSE_SHAPES))
def test_joint_mean_cov(ext, dense_ops, shape):
  case = qc.dense_case(*shape)
  ref = qc.dense_reference(*shape)
  tol_mean, tol_cov = qc.joint_bounds(case, ref)
  mean, cov, dist = (t.cpu() for t in dense_ops[shape].joint(ext))
  assert mean.shape == (case.b, case.q)
  assert cov.shape == (case.b, case.q, case.q)
  assert dist.shape == (case.b,)
  e_mean = (mean.double() - ref.mean).abs()
  e_cov = (cov.double() - ref.cov).abs()
  print(f'OBSERVED joint {shape}: mean {float(e_mean.max()):.3e} (bound '
        f'{float(tol_mean.min()):.3e}), cov {float(e_cov.max()):.3e} '
        f'(bound {float(tol_cov.min()):.3e})')
  assert bool((e_mean <= tol_mean).all()), (e_mean / tol_mean).max()
  assert bool((e_cov <= tol_cov).all()), (e_cov / tol_cov).max()
  assert torch.equal(cov, cov.transpose(1, 2))
  # The kernel writes amp^2 on the diagonal of kqq: diag = amp^2 - Q.
  assert bool((cov.diagonal(dim1=1, dim2=2) < sc.AMP2_F32).all())
  assert bool(((dist.double() - ref.dist).abs() <=
               2.0 ** -23 * ref.dist).all())


# -- 2. spikes ---------------------------------------------------------------------


@pytest.mark.parametrize('shape', qc.SPIKE_SHAPES, ids=_ids(qc.SPIKE_SHAPES))
def test_joint_spikes(ext, shape):
  case = qc.make_spike_case(*shape)
  ops = Ops(case)
  k = qc.joint_reference(case).k                        # (b, q, n) fp64
  alpha = torch.zeros(case.n, device=DEV)
  kinv = torch.zeros(case.n, case.n, device=DEV)
  # Kinv = 0 gives the kernel's own kqq, so that Q = kqq - cov carries the
  # rounding of one subtraction and not the error of kqq.
  mean0, kqq, _ = ops.joint(ext, alpha=alpha, kinv=kinv)
  assert torch.equal(mean0.cpu(), torch.full((case.b, case.q), sc.MEAN_C))
  worst_mu = worst_q = 0.0
  for i, j in qc.spike_pairs(case.n):
    alpha[i] = 1.0
    kinv[i, j] = sc.SPIKE_C
    kinv[j, i] = sc.SPIKE_C
    mean, cov, _ = ops.joint(ext, alpha=alpha, kinv=kinv)
    alpha[i] = 0.0
    kinv[i, j] = 0.0
    kinv[j, i] = 0.0
    got_q = (kqq - cov).cpu().double()
    c = sc.SPIKE_C if i != j else 0.5 * sc.SPIKE_C
    want_q = c * (k[:, :, None, i] * k[:, None, :, j] +
                  k[:, :, None, j] * k[:, None, :, i])
    want_mu = k[:, :, i]
    e_mu = ((mean.cpu().double() - sc.MEAN_C) - want_mu).abs() / want_mu
    e_q = (got_q - want_q).abs() / want_q
    worst_mu = max(worst_mu, float(e_mu.max()))
    worst_q = max(worst_q, float(e_q.max()))
    assert float(e_mu.max()) <= sc.TOL_SPIKE_REL, (i, j)
    assert float(e_q.max()) <= sc.TOL_SPIKE_REL, (i, j)
  print(f'OBSERVED spikes {shape}: mean {worst_mu:.3e}, quad {worst_q:.3e} '
        f'(bound {sc.TOL_SPIKE_REL:.1e})')


# -- 3. Cholesky + Monte-Carlo stage on hand-made covariances ----------------------


def _eps(s, q, seed):
  g = torch.Generator().manual_seed(seed)
  return torch.randn(s, q, generator=g, dtype=torch.float64).float()


@pytest.mark.parametrize('s', qc.SAMPLES)
def test_mc_diagonal_q1(ext, s):
  eps = _eps(s, 1, 5)
  var = torch.tensor([0.01, 1.0, 7.5, 1e-6])
  sd = (var.double() * (1.0 + 1e-4)).sqrt()
  y = sd[None, :] * eps.double()                         # (S, B)
  want = y.clamp_min(0).mean(0)
  got = ext.qei_scores_from_cov(
      torch.zeros(4, 1, device=DEV), var.view(4, 1, 1).to(DEV),
      eps.to(DEV), 0.0).cpu().double()
  tol = 1 * 2.0 ** -22 * y.abs().amax(0)
  err = (got - want).abs()
  print(f'OBSERVED mc diagonal S={s}: {float((err / tol).max()):.3f} of '
        'the bound')
  assert bool((err <= tol).all())


def test_mc_sampling_covariance_is_correct(ext):
  # The statistic of test_gp_core.py::
  # test_qei_mc_sampling_covariance_is_correct, for the kernel: the score is
  # the MC qEI of y = L eps, not of L^T eps.
  torch.manual_seed(0)
  cov = torch.tensor([[[1.0, 0.9], [0.9, 1.0]]])
  mean = torch.zeros(1, 2)
  eps = torch.randn(200000, 2)
  L = torch.linalg.cholesky(cov.double() + 1e-4 * torch.eye(2).double())
  y = torch.einsum('sc,brc->sbr', eps.double(), L)[:, 0, :]
  emp = (y.T @ y) / y.shape[0]
  assert torch.allclose(emp, cov[0].double(), atol=0.05), emp
  want = float(y.clamp_min(0).amax(-1).mean())
  y_t = torch.einsum('sc,bcr->sbr', eps.double(), L)[:, 0, :]
  wrong = float(y_t.clamp_min(0).amax(-1).mean())
  assert abs(wrong - want) > 1e-2 * want     # the check can tell them apart
  got = float(ext.qei_scores_from_cov(mean.to(DEV), cov.to(DEV),
                                      eps.to(DEV), 0.0)[0])
  print(f'OBSERVED mc covariance: kernel {got:.7f}, fp64 {want:.7f}, '
        f'transposed {wrong:.7f}')
  assert got == pytest.approx(want, rel=1e-4)


NAN = float('nan')
BAD_COVS = [[[1.0, 2.0], [2.0, 1.0]],           # indefinite
            [[0.5, NAN], [NAN, 2.0]]]           # NaN off-diagonals
GOOD_COVS = [[[1.0, 0.3], [0.3, 0.5]], [[2.0, -1.0], [-1.0, 1.5]],
             [[0.2, 0.0], [0.0, 0.1]]]


def _marginals(mean, cov, eps, best):
  """fp64 fallback value: diagonal marginals of the UN-jittered diagonal."""
  sd = cov.double().diagonal(dim1=-2, dim2=-1).sqrt()
  y = mean.double()[None] + sd[None] * eps.double()[:, None, :]
  return (y - best).clamp_min(0).amax(-1).mean(0)


@pytest.mark.parametrize('s', qc.SAMPLES)
def test_mc_fallback_values(ext, s):
  eps = _eps(s, 2, 6)
  cov = torch.tensor(BAD_COVS)
  mean = torch.tensor([[0.1, -0.2], [0.0, 0.3]])
  best = 0.05
  want = qc.mc_scores(mean, cov, eps, best)
  assert torch.isfinite(want).all()
  assert torch.allclose(want, _marginals(mean, cov, eps, best), rtol=0,
                        atol=1e-15)
  got = ext.qei_scores_from_cov(mean.to(DEV), cov.to(DEV), eps.to(DEV),
                                best).cpu().double()
  tol = qc.mc_floor(2, mean, cov, eps)
  err = float((got - want).abs().max())
  print(f'OBSERVED mc fallback S={s}: {err:.3e} (bound {tol:.3e})')
  assert err <= tol


def test_mc_fallback_does_not_leak_across_sets(ext):
  eps = _eps(qc.S_MAX, 2, 7)
  covs = [GOOD_COVS[0], BAD_COVS[0], GOOD_COVS[1], BAD_COVS[1], GOOD_COVS[2]]
  cov = torch.tensor(covs)
  g = torch.Generator().manual_seed(8)
  mean = (torch.rand(5, 2, generator=g, dtype=torch.float64) - 0.5).float()
  best = 0.05
  assert qc.uses_fallback(cov.double()).tolist() == [False, True, False,
                                                     True, False]
  want = qc.mc_scores(mean, cov, eps, best)
  got = ext.qei_scores_from_cov(mean.to(DEV), cov.to(DEV), eps.to(DEV),
                                best).cpu()
  tol = qc.mc_floor(2, mean, cov, eps)
  err = float((got.double() - want).abs().max())
  print(f'OBSERVED mc mixed batch: {err:.3e} (bound {tol:.3e})')
  assert err <= tol
  # A good set scores the same, bit for bit, with or without bad neighbours.
  good = [0, 2, 4]
  alone = ext.qei_scores_from_cov(
      mean[good].to(DEV), cov[good].to(DEV), eps.to(DEV), best).cpu()
  assert torch.equal(alone, got[good])


# -- 3e / 4. measured margin on the dense shapes ------------------------------------


@pytest.fixture(scope='module')
def family(ext, dense_ops):
  """Kernel and fp32-torch errors over the whole (shape, S) family.

  mc:  the kernel's OWN fp32 (mean, cov) through fp64 qei_mc_scores is the
       reference for both qei_scores_from_cov and fp32 torch qei_mc_scores
       on the GPU.
  e2e: the fp64 reference of the case is the reference for both
       qei_set_scores and fp32 torch posterior_batched_cov + qei_mc_scores
       on the GPU.
  """
  from vizier_amd._src.algorithms.designers.gp_bandit import (
      posterior_batched_cov,
  )
  from vizier_amd._src.gp import acquisitions as acq_lib
  rows = {}
  for shape in qc.DENSE_SHAPES:
    case, ops = qc.dense_case(*shape), dense_ops[shape]
    ref = qc.dense_reference(*shape)
    mean, cov, _ = ops.joint(ext)
    t_mean, t_cov = posterior_batched_cov(
        case.posterior(torch.float32, DEV), ops.xs)
    for s in qc.SAMPLES:
      eps = ops.eps[:s].contiguous()
      want_mc = qc.mc_scores(mean, cov, eps, case.best)
      want_e2e = qc.mc_scores(ref.mean, ref.cov, eps, case.best)

      def err(got, want):
        return float((got.cpu().double() - want).abs().max())
      rows[shape, s] = dict(
          mc_kernel=err(ext.qei_scores_from_cov(mean, cov, eps, case.best),
                        want_mc),
          mc_torch=err(acq_lib.qei_mc_scores(mean, cov, eps, case.best),
                       want_mc),
          mc_floor=qc.mc_floor(case.q, mean, cov, eps),
          e2e_kernel=err(ops.scores(ext, s), want_e2e),
          e2e_torch=err(acq_lib.qei_mc_scores(t_mean, t_cov, eps, case.best),
                        want_e2e),
          e2e_floor=qc.mc_floor(case.q, ref.mean, ref.cov, eps))
  return rows


@pytest.mark.parametrize('stage', ['mc', 'e2e'])
def test_dense_scores_within_measured_margin(family, stage):
  torch_max = max(r[f'{stage}_torch'] for r in family.values())
  kernel_max = max(r[f'{stage}_kernel'] for r in family.values())
  print(f'OBSERVED {stage}: fp32 torch max error {torch_max:.3e} (margin '
        f'4x = {4 * torch_max:.3e}), kernel max error {kernel_max:.3e}')
  for (shape, s), r in family.items():
    tol = max(4.0 * torch_max, r[f'{stage}_floor'])
    print(f'  {stage} {shape} S={s}: kernel {r[f"{stage}_kernel"]:.3e}, '
          f'torch {r[f"{stage}_torch"]:.3e}, floor '
          f'{r[f"{stage}_floor"]:.3e}, tolerance {tol:.3e}')
  for (shape, s), r in family.items():
    tol = max(4.0 * torch_max, r[f'{stage}_floor'])
    assert r[f'{stage}_kernel'] <= tol, (shape, s)


def test_set_scores_are_deterministic(ext, dense_ops):
  ops = dense_ops[25, 8, 257, 20]
  first, second = ops.scores(ext, 128), ops.scores(ext, 128)
  assert torch.equal(first, second)
  a, b = ops.joint(ext), ops.joint(ext)
  for u, v in zip(a, b):
    assert torch.equal(u, v)


@pytest.mark.parametrize('shape', qc.TR_SHAPES, ids=_ids(qc.TR_SHAPES))
def test_trust_region_is_decided_by_member_zero(ext, family, shape):
  b, q, n, nearest = shape
  case = qc.make_tr_case(b, q, n, nearest)
  ops = Ops(case, onehot=sc.TR_ONEHOT)
  want = qc.set_scores_reference(case, qc.S_MAX,
                                 trust_region=qc.trust_region(case))
  got = ops.scores(ext, qc.S_MAX, tr_radius=sc.TR_RADIUS)
  assert torch.equal(got, ops.scores(ext, qc.S_MAX, tr_radius=sc.TR_RADIUS))
  got = got.cpu().double()
  h = b // 2
  ref = qc.joint_reference(case)
  tol = max(4.0 * max(r['e2e_torch'] for r in family.values()),
            qc.mc_floor(q, ref.mean, ref.cov, case.eps))
  e_in = float((got[:h] - want[:h]).abs().max())
  e_out = float((got[h:] - want[h:]).abs().max())
  print(f'OBSERVED trust region {shape}: inside {e_in:.3e} (bound '
        f'{tol:.3e}), penalised {e_out:.3e} (bound {sc.TOL_PENALTY:.1e})')
  assert bool((got[:h] >= 0).all()) and bool((got[h:] < -1e4).all())
  assert e_in <= tol
  assert e_out <= sc.TOL_PENALTY
  # No trust region (radius 0) scores every set.
  assert bool((ops.scores(ext, qc.S_MAX) >= 0).all())


# -- argument checks ---------------------------------------------------------------


def _small_args(q=2, d=3, n=8, s=4, eps_q=None):
  z = lambda *shape: torch.zeros(*shape, device=DEV)
  return (torch.rand(2, q, d, device=DEV), torch.rand(n, d, device=DEV),
          torch.ones(d, device=DEV), 1.0, 0.0, z(n), z(n, n),
          torch.zeros(d, dtype=torch.uint8, device=DEV),
          torch.randn(s, q if eps_q is None else eps_q, device=DEV), 0.0,
          0.0)


def test_limits_raise(ext):
  assert ext.qei_set_scores(*_small_args(q=16)).shape == (2,)
  assert ext.qei_set_scores(*_small_args(d=512)).shape == (2,)
  with pytest.raises(RuntimeError, match='q <= 16'):
    ext.qei_set_scores(*_small_args(q=17))
  with pytest.raises(RuntimeError, match='q <= 16'):
    ext.qei_joint_mean_cov(*_small_args(q=17)[:8])
  with pytest.raises(RuntimeError, match='D <= 512'):
    ext.qei_set_scores(*_small_args(d=513))
  with pytest.raises(RuntimeError, match='eps'):
    ext.qei_set_scores(*_small_args(q=2, eps_q=3))
  z = lambda *shape: torch.zeros(*shape, device=DEV)
  with pytest.raises(RuntimeError, match='eps'):
    ext.qei_scores_from_cov(z(2, 2), z(2, 2, 2), z(4, 3), 0.0)
  with pytest.raises(RuntimeError, match='q <= 16'):
    ext.qei_scores_from_cov(z(2, 17), z(2, 17, 17), z(4, 17), 0.0)
  with pytest.raises(RuntimeError, match='cov'):
    ext.qei_scores_from_cov(z(2, 2), z(2, 3, 3), z(4, 2), 0.0)
  with pytest.raises(RuntimeError, match='sample'):
    ext.qei_scores_from_cov(z(2, 2), z(2, 2, 2), z(0, 2), 0.0)


# -- 5. the designer: capture and the suggest loop -------------------------------------


def _problem():
  from vizier_amd import pyvizier as vz
  problem = vz.ProblemStatement()
  for i in range(4):
    problem.search_space.root.add_float_param(f'x{i}', 0.0, 1.0)
  problem.metric_information.append(vz.MetricInformation(
      name='obj', goal=vz.ObjectiveMetricGoal.MAXIMIZE))
  return problem


def _fitted_designer(n_trials=24, **kw):
  from vizier_amd import pyvizier as vz
  from vizier_amd._src.algorithms.core.abstractions import (
      ActiveTrials,
      CompletedTrials,
  )
  from vizier_amd._src.algorithms.designers.gp_bandit import (
      GPBanditConfig,
      VizierGPBandit,
  )
  d = VizierGPBandit(_problem(), GPBanditConfig(
      acquisition='qei', ard_restarts=1, ard_max_iters=10, device='cuda',
      **kw), seed=1)
  rng = np.random.default_rng(0)
  trials = []
  for uid in range(1, n_trials + 1):
    params = {f'x{i}': float(rng.uniform()) for i in range(4)}
    t = vz.Trial(params, id=uid)
    t.complete(vz.Measurement(
        metrics={'obj': -sum((v - 0.5) ** 2 for v in params.values())}))
    trials.append(t)
  d.update(CompletedTrials(trials), ActiveTrials())
  d._fit()
  return d


def _sweep(d, score_fn, q):
  """optimizer.optimize(count=1) built the way _gp_suggestions builds it."""
  from vizier_amd._src.algorithms.optimizers.eagle import (
      CandidateBatch,
      EagleStrategyConfig,
  )
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
          seed=d._seed + len(d._trials), device=d._device, dtype=cfg.dtype)
  dense = torch.as_tensor(d._x_cache, dtype=cfg.dtype, device=d._device)
  prior = d._codec.encode(dense)
  rewards = d._warped_labels[:, 0].to(d._device, cfg.dtype)
  groups = prior.continuous.shape[0] // q
  prior = CandidateBatch(
      prior.continuous[:groups * q, 0, :].reshape(groups, q, -1).contiguous(),
      prior.categorical[:groups * q, 0, :].reshape(groups, q,
                                                   -1).contiguous())
  rewards = rewards[:groups * q].reshape(groups, q).amax(dim=1)
  results = optimizer.optimize(score_fn, count=1, prior_features=prior,
                               prior_rewards=rewards)
  return optimizer, results


def test_hip_scorer_sweep_is_captured_and_matches_eager(ext):
  d = _fitted_designer(qei_scorer='hip', max_evaluations=2000)
  score_fn, q = d._score_factory(4)
  assert q == 4
  assert score_fn.graph_safe is True
  captured, got = _sweep(d, score_fn, q)
  assert captured.last_used_graph is True
  assert captured.last_graph_error is None

  def eager_fn(batch):
    return score_fn(batch)
  eager_fn.graph_safe = False          # forces the eager loop
  eager, want = _sweep(d, eager_fn, q)
  assert eager.last_used_graph is False
  # count = 1: the final-pool selection of the captured sweep is exact.
  assert torch.equal(got.rewards, want.rewards)
  assert torch.equal(got.features.continuous, want.features.continuous)
  assert got.features.continuous.shape == (1, 4, 4)
  # The process is not left in capture mode.
  assert float(torch.ones(8, device=DEV).sum()) == 8.0
  assert not torch.cuda.is_current_stream_capturing()


def test_default_scorer_is_still_not_offered_for_capture(ext):
  d = _fitted_designer(max_evaluations=200)
  score_fn, q = d._score_factory(4)
  assert q == 4 and score_fn.graph_safe is False
  # More members than the kernels take: the torch set scorer.
  d = _fitted_designer(qei_scorer='hip', max_evaluations=200)
  score_fn, q = d._score_factory(17)
  assert q == 17 and score_fn.graph_safe is False


def test_hip_scorer_with_linear_kernel_stays_eager(ext):
  # LinearMaternPosterior: torch joint covariance + the HIP Cholesky /
  # Monte-Carlo stage; not capturable.
  d = _fitted_designer(qei_scorer='hip', max_evaluations=200,
                       linear_coef=1.0)
  score_fn, q = d._score_factory(3)
  assert score_fn.graph_safe is False
  assert len(d.suggest(3)) == 3


def test_hip_scorer_suggest_loop(ext):
  from vizier_amd import pyvizier as vz
  from vizier_amd._src.algorithms.core.abstractions import (
      ActiveTrials,
      CompletedTrials,
  )
  from vizier_amd._src.algorithms.designers.gp_bandit import (
      GPBanditConfig,
      VizierGPBandit,
  )
  d2 = VizierGPBandit(_problem(), GPBanditConfig(
      max_evaluations=1500, acquisition='qei', qei_scorer='hip',
      ard_restarts=1, ard_max_iters=10, device='cuda'), seed=1)
  uid = 0
  for _ in range(4):
    batch = d2.suggest(3)
    assert len(batch) == 3
    rows = [tuple(round(s.parameters.get_value(f'x{i}'), 6)
                  for i in range(4)) for s in batch]
    assert len(set(rows)) == 3, 'qEI produced identical batch points'
    trials = []
    for s in batch:
      uid += 1
      x = np.array([s.parameters.get_value(f'x{i}') for i in range(4)])
      t = s.to_trial(uid)
      t.complete(vz.Measurement(
          metrics={'obj': float(-((x - 0.5) ** 2).sum())}))
      trials.append(t)
    d2.update(CompletedTrials(trials), ActiveTrials())
