"""Fused separable-multitask scorer (posterior_score_multitask.hip) against
the float64 MultitaskFusedCache formula; the cache against predict(); the
`multitask_scorer` knob. Kernel operands: seeded, x and xq uniform in the unit
box, lengthscales in [0.3, 1] * max(1, sqrt(d / 4)), task scales in
[0.5, 1.5], B from a random correlation Cholesky ('diag': no correlation,
'rank1': one column), tau = 1e-2 max B_tt, a_mat scaled like scorer_cases'
alpha. Asserted on the reference alone: every variance >= 1e-3 of its prior,
every candidate's largest k >= 0.05. Worst observed error / bound: README.
"""

import functools

import numpy as np
import pytest
import torch

import scorer_cases as sc
from vizier_amd._src.gp import multitask as mt
from vizier_amd._src.gp.matern import gram_matern52

U = 2.0 ** -24
SHAPES = [(1, 1, 1, 2), (3, 63, 4, 2), (25, 64, 3, 3), (25, 65, 3, 3),
          (32, 130, 5, 4), (33, 70, 4, 2), (4, 70, 64, 2), (4, 70, 65, 2),
          (2, 70, 512, 2), (4, 70, 3, 8), (25, 1100, 8, 2),
          (25, 70, 3, 'diag'), (25, 70, 3, 'rank1')]
TR_SHAPE = (24, 70, 16, 2)
TR_ONEHOT = (0, 0, 1, 1, 1, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0)


def _task_chol(r, kind):
  m = 3 if isinstance(kind, str) else kind
  lc = torch.tril(2.0 * r(m, m) - 1.0, -1) + torch.eye(m).double()
  if kind == 'diag':
    lc = torch.eye(m).double()
  elif kind == 'rank1':
    lc = torch.cat([torch.ones(m, 1), torch.zeros(m, m - 1)], 1).double()
  lc = lc / lc.norm(dim=-1, keepdim=True)
  return (0.5 + r(m)).unsqueeze(-1) * lc


def _formula(f, x, xq):
  """(mean, var, k) of the cache `f`, in f's dtype."""
  k = gram_matern52(xq.to(f.w.dtype), x.to(f.w.dtype), f.lengthscales,
                    torch.ones((), dtype=f.w.dtype))
  quad = torch.einsum('qi,sij,qj->qs', k, f.w, k)
  return f.means + k @ f.a_mat, f.bdiag - quad @ f.c.T, k


@functools.lru_cache(maxsize=None)
def _case(b, n, d, kind, onehot=None):
  """Operands, float64 reference and CPU fp32 errors: built once, shared."""
  g = torch.Generator().manual_seed(1000 * b + n + 7 * d)
  r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
  x = r(n, d).float()
  ls = (0.3 + 0.7 * r(d)) * max(1.0, (d / 4.0) ** 0.5)
  mask = [0] * d if onehot is None else list(onehot)
  if onehot is None:
    xq = r(b, d).float()
  else:  # half the candidates inside the 0.3 radius, half outside
    pool = r(16 * b, d).float()
    far = sc.min_linf_dist(pool, x, mask) > 0.3
    xq = torch.cat([pool[~far][:b // 2], pool[far][:b - b // 2]])
  chol = _task_chol(r, kind)
  m = chol.shape[0]
  tau = 1e-2 * (chol @ chol.T).diagonal().max()
  params = mt.MultitaskParams(noise=tau, means=r(m) - 0.5, lengthscales=ls,
                              task_chol=chol)
  f64 = mt._build_fused_cache(x.double(), params, torch.zeros(n, m).double(),
                              tau)
  sign = torch.where(r(n, m) < 0.5, -1.0, 1.0).double()
  f64.a_mat = sign * (0.5 + 0.5 * r(n, m)) / n ** 0.5
  f32 = mt.MultitaskFusedCache(**{
      k: v.float() if torch.is_tensor(v) else v
      for k, v in vars(f64).items()})
  assert torch.equal(f32.w, f32.w.mT)
  mean, var, k = _formula(f64, x, xq)
  assert bool((var >= 1e-3 * f64.bdiag).all())
  assert float(k.max(-1).values.min()) >= 0.05
  m32, v32, _ = _formula(f32, x, xq)
  ka = k.abs()
  absquad = torch.einsum('qi,sij,qj->qs', ka, f64.w.abs(), ka)
  return dict(
      x=x, xq=xq, onehot=mask, f=f32, mean=mean, var=var,
      dist=sc.min_linf_dist(xq, x, mask),
      tol_mean=4 * float((m32 - mean).abs().max()) +
      8 * U * (ka @ f64.a_mat.abs()),
      tol_var=4 * float((v32 - var).abs().max()) +
      8 * U * (absquad @ f64.c.T + f64.bdiag))


def _call(case, **over):
  from vizier_amd._src.ops import dispatch
  f = case['f']
  a = dict(xq=case['xq'], x=case['x'], lengthscales=f.lengthscales,
           means=f.means, a_mat=f.a_mat, w=f.w, c=f.c, bdiag=f.bdiag)
  a = {k: v.cuda() for k, v in a.items()}
  a['onehot'] = torch.tensor(case['onehot'], dtype=torch.uint8).cuda()
  a.update(over)
  out = dispatch.require_ext().multitask_mean_std(*a.values())
  return [t.cpu() for t in out]


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES + [TR_SHAPE], ids=str)
def test_means_sds_dist_against_float64(shape):
  c = _case(*shape, TR_ONEHOT if shape == TR_SHAPE else None)
  means, sds, dist = _call(c)
  assert bool(torch.isfinite(means).all() and torch.isfinite(sds).all())
  e_mean = float(((means.T.double() - c['mean']).abs() / c['tol_mean']).max())
  e_var = float(((sds.T.double() ** 2 - c['var']).abs() / c['tol_var']).max())
  print(f'OBSERVED {shape}: error / bound {e_mean:.3f} (mean), '
        f'{e_var:.3f} (variance)')
  assert e_mean <= 1.0 and e_var <= 1.0
  assert torch.equal(dist, c['dist'])
  if shape == TR_SHAPE:
    assert int((dist > 0.3).sum()) == shape[0] // 2


@pytest.mark.gpu
@pytest.mark.parametrize('bad', [
    'cpu', 'dtype', 'strided', 'a_mat', 'w_not_square', 'm9', 'n4096',
    'd513'])
def test_binding_rejects_malformed_operands(bad):
  c = _case(3, 63, 4, 2)
  z = lambda *s: torch.zeros(*s, device='cuda')
  over = {
      'cpu': dict(xq=c['xq']),
      'dtype': dict(x=c['x'].double().cuda()),
      'strided': dict(xq=torch.rand(3, 8).cuda()[:, ::2]),
      'a_mat': dict(a_mat=z(62, 2)),
      'w_not_square': dict(w=z(2, 63, 62)),
      'm9': dict(w=z(9, 63, 63), a_mat=z(63, 9), c=z(9, 9), bdiag=z(9),
                 means=z(9)),
      'n4096': dict(x=z(4096, 4), w=z(1, 4096, 4096), a_mat=z(4096, 1),
                    c=z(1, 1), bdiag=z(1), means=z(1)),
      'd513': dict(x=z(63, 513), xq=z(3, 513), lengthscales=z(513) + 1,
                   onehot=z(513).to(torch.uint8))}[bad]
  with pytest.raises(RuntimeError):
    _call(c, **over)


def _params(kind, like):
  g = torch.Generator().manual_seed(5)
  r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
  to = lambda t: t.to(like)
  return mt.MultitaskParams(
      noise=to(torch.tensor(1e-4)), means=to(r(2 if kind == 2 else 3) - 0.5),
      lengthscales=to(0.3 + 0.7 * r(like.shape[1])),
      task_chol=to(_task_chol(r, kind)))


@pytest.mark.parametrize('kind', [3, 'diag', 'rank1'])
def test_float64_cache_formula_equals_predict(kind):
  g = torch.Generator().manual_seed(7)
  x, xq = (torch.rand(s, 4, generator=g, dtype=torch.float64)
           for s in (60, 33))
  y = torch.randn(60, 3, generator=g, dtype=torch.float64)
  post = mt.posterior_from_params(x, y, _params(kind, x),
                                  with_fused_cache=True)
  assert mt.posterior_from_params(x, y, post.params).fused is None
  want_mean, want_sd = post.predict(xq)
  mean, var, _ = _formula(post.fused, x, xq)
  assert bool(((mean - want_mean).abs() <= 1e-9 * want_mean.abs()).all())
  assert bool(((var - want_sd ** 2).abs() <= 1e-9 * post.fused.bdiag).all())


def _designer(name, monkeypatch, pending=False, **kw):
  """A two-metric 4-D study with its posterior installed, not fitted."""
  from vizier_amd import pyvizier as vz
  from vizier_amd._src.algorithms.core import abstractions as ab
  from vizier_amd._src.algorithms.designers import gp_bandit, gp_ucb_pe
  monkeypatch.setattr(
      mt, 'train_multitask_gp',
      lambda x, y, with_fused_cache=False, **_: mt.posterior_from_params(
          x, y, _params(2, x), with_fused_cache=with_fused_cache))
  problem = vz.ProblemStatement()
  for i in range(4):
    problem.search_space.root.add_float_param(f'x{i}', 0.0, 1.0)
  for name_ in ('a', 'b'):
    problem.metric_information.append(vz.MetricInformation(
        name=name_, goal=vz.ObjectiveMetricGoal.MAXIMIZE))
  cls, cfg = {
      'bandit': (gp_bandit.VizierGPBandit, gp_bandit.GPBanditConfig),
      'ucb_pe': (gp_ucb_pe.VizierGPUCBPEBandit, gp_ucb_pe.UCBPEConfig)}[name]
  kw.setdefault('device', 'cuda')
  d = cls(problem, cfg(multitask_type='separable', max_evaluations=2000,
                       **kw), seed=1)
  trials = []
  for uid, v in enumerate(np.random.default_rng(0).uniform(size=(70, 4)), 1):
    trials.append(vz.Trial({f'x{i}': float(v[i]) for i in range(4)}, id=uid))
    trials[-1].complete(vz.Measurement(
        metrics={'a': float(-((v - 0.3) ** 2).sum()),
                 'b': float(-((v - 0.6) ** 2).sum())}))  # interior optimum
  active = [vz.Trial({f'x{i}': 0.5 for i in range(4)}, id=99)] * pending
  d.update(ab.CompletedTrials(trials), ab.ActiveTrials(active))
  d._fit()
  if name == 'bandit':
    return d, d._mt_posterior, d._score_factory(1)[0]
  x_all = d._posterior.x
  if pending:
    x_all = torch.cat([x_all, torch.full((1, 4), 0.5, device=x_all.device)])
  return d, d._mo_posteriors[0]._mt, d._one_score_fn(True, x_all)


@pytest.mark.parametrize('name', ['bandit', 'ucb_pe'])
def test_unknown_scorer_cpu_and_float64_raise(name, monkeypatch):
  with pytest.raises(ValueError, match='multitask_scorer'):
    _designer(name, monkeypatch, multitask_scorer='bogus', device='cpu')
  with pytest.raises(ValueError, match='GPU device'):
    _designer(name, monkeypatch, multitask_scorer='hip', device='cpu')


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['bandit', 'ucb_pe'])
def test_designer_engages_and_captures_the_hip_scorer(name, monkeypatch):
  from vizier_amd._src.algorithms.optimizers import eagle, vectorized
  from vizier_amd._src.gp import acquisitions as acq_lib
  from vizier_amd._src.ops import dispatch
  with pytest.raises(ValueError, match='float32'):
    _designer(name, monkeypatch, multitask_scorer='hip', dtype=torch.float64)
  _, post, torch_fn = _designer(name, monkeypatch)
  assert post.fused is None and torch_fn.graph_safe is False
  d, post, score_fn = _designer(name, monkeypatch, multitask_scorer='hip')
  assert score_fn.graph_safe is True
  if name == 'ucb_pe':  # a pending trial: the trust region is not anchored
    assert _designer(name, monkeypatch, pending=True,
                     multitask_scorer='hip')[2].graph_safe is False

  ext, f, cfg = dispatch.require_ext(), post.fused, d._config
  dense = torch.rand(25, 4, generator=torch.Generator().manual_seed(3)).cuda()
  tr = acq_lib.TrustRegion.for_converter(post.x, d._converter)
  scal = d._mo_scalarizer if name == 'ucb_pe' else \
      acq_lib.create_hv_scalarization(
          cfg.num_scalarizations, 2, seed=d._seed,
          reference_point=acq_lib.get_reference_point(
              d._warped_labels, scale=cfg.ref_scaling))
  means, sds, dist = ext.multitask_mean_std(
      dense, post.x, f.lengthscales, f.means, f.a_mat, f.w, f.c, f.bdiag,
      tr._onehot.to(torch.uint8))
  want = ext.hv_scalarize_tr(
      means, sds, scal.weights.float().cuda().contiguous(),
      scal.reference_point.float().cuda().contiguous(), dist,
      cfg.ucb_coefficient, float(tr.trust_radius))
  assert torch.equal(score_fn(d._codec.encode(dense)), want)
  def sweep(fn):
    optimizer = vectorized.VectorizedOptimizerFactory(
        eagle_config=eagle.EagleStrategyConfig(), max_evaluations=2000,
        suggestion_batch_size=25)(
            n_continuous=d._codec.n_continuous,
            categorical_sizes=d._codec.categorical_sizes, seed=5,
            device=d._device, dtype=torch.float32)
    return optimizer, optimizer.optimize(fn, count=1)
  captured, got = sweep(score_fn)
  assert captured.last_used_graph is True and captured.last_graph_error is None
  eager_fn = lambda batch: score_fn(batch)
  eager_fn.graph_safe = False
  eager, want = sweep(eager_fn)
  assert eager.last_used_graph is False
  assert torch.equal(got.rewards, want.rewards)
  assert torch.equal(got.features.continuous, want.features.continuous)
