"""Fused Matern + linear kernel scorer (posterior_score_linear.hip) against
the float64 `LinearMaternPosterior.predict` formula; the `linear_scorer` knob
and the `K_inv_lin` cache. Kernel operands: seeded, uniform in the unit box,
lengthscales in [0.3, 1], noise 1e-2 amp^2, shift 0.2, linear term ~ amp^2
('strong') or 30x smaller ('weak'), float64 torch.linalg.inv; alpha as in
scorer_cases (the kernel takes any). Asserted on the reference alone: every
variance >= 1e-3 of its prior. At (25, 4100, 3) no seed can give that (4100
rows in a 3-D box put hundreds within a lengthscale of every candidate, so
the variance is ~ noise / that count: 1.3e-4 and 2.9e-4 of the prior here);
that shape asserts 1e-4. Worst observed error / bound: see the README.
"""

import functools

import numpy as np
import pytest
import torch

import scorer_cases as sc
from vizier_amd._src.gp import linear_matern as lm

AMP, MEAN_C, SHIFT, U = sc.AMP, sc.MEAN_C, 0.2, 2.0 ** -24
SHAPES = [(1, 1, 1), (3, 63, 4), (25, 64, 3), (25, 65, 3), (32, 130, 5),
          (33, 70, 4), (4, 70, 64), (4, 70, 65), (2, 70, 512), (25, 4100, 3)]
TR_SHAPE = (24, 70, 16)
TR_ONEHOT = (0, 0, 1, 1, 1, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0)
# scorer_cases' tolerance presumes sd >= 0.7 amp: the table's shapes that
# meet it on the reference.
SCORE_SHAPES = [(4, 70, 65), (2, 70, 512)]


def _predict(c, dtype, kinv=None):
  """(mean, var, prior, k, kinv) by the predict formula in `dtype`."""
  t = functools.partial(torch.tensor, dtype=dtype)
  p = lm.LinearMaternParams(t(AMP), t(1e-2 * AMP * AMP), t(MEAN_C),
                            t(c['slope']), t(SHIFT), c['ls'].to(dtype))
  x, xq = c['x'].to(dtype), c['xq'].to(dtype)
  k = lm._combined_gram(p, 1.0, xq, x)
  if kinv is None:
    gram = lm._combined_gram(p, 1.0, x, None)
    kinv = torch.linalg.inv(gram + p.noise * torch.eye(len(x), dtype=dtype))
  zq = xq / p.lengthscales - SHIFT
  prior = p.amplitude ** 2 + p.slope ** 2 * (zq * zq).sum(-1)
  mean = MEAN_C + k @ c['alpha'].to(dtype)
  return mean, prior - (k * (k @ kinv)).sum(-1), prior, k, kinv


@functools.lru_cache(maxsize=None)
def _case(b, n, d, weak, onehot=None):
  """Operands, float64 reference and CPU fp32 errors: built once, shared."""
  g = torch.Generator().manual_seed(1000 * b + n + 7 * d)
  r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
  x, ls = r(n, d).float(), (0.3 + 0.7 * r(d)).float()
  mask = [0] * d if onehot is None else list(onehot)
  if onehot is None:
    xq = r(b, d).float()
  else:  # half the candidates inside the 0.3 radius, half outside
    pool = r(16 * b, d).float()
    far = sc.min_linf_dist(pool, x, mask) > 0.3
    xq = torch.cat([pool[~far][:b // 2], pool[far][:b - b // 2]])
  sign = torch.where(r(n) < 0.5, -1.0, 1.0).double()
  z = x.double() / ls.double() - SHIFT
  slope = AMP / (float((z * z).sum(-1).mean()) * (30 if weak else 1)) ** 0.5
  c = dict(x=x, xq=xq, ls=ls, slope=slope, onehot=mask,
           alpha=(sign * (0.5 + 0.5 * r(n)) / n ** 0.5).float())
  mean, var, prior, k, kinv = _predict(c, torch.float64)
  assert bool((var >= (1e-4 if n == 4100 else 1e-3) * prior).all())
  c.update(mean=mean, var=var, prior=prior, kinv=kinv.float(),
           dist=sc.min_linf_dist(xq, x, mask))
  m32, v32, _, _, _ = _predict(c, torch.float32, c['kinv'])
  ka = k.abs()
  c['tol_mean'] = 4 * float((m32 - mean).abs().max()) + \
      8 * U * (ka @ c['alpha'].double().abs())
  c['tol_var'] = 4 * float((v32 - var).abs().max()) + \
      8 * U * (((ka @ kinv.abs()) * ka).sum(-1) + prior)
  return c


def _call(name, c, *tail, **over):
  from vizier_amd._src.ops import dispatch
  a = {k: c[k].cuda() for k in ('xq', 'x', 'ls', 'alpha', 'kinv')}
  a['onehot'] = torch.tensor(c['onehot'], dtype=torch.uint8).cuda()
  a.update(over)
  out = getattr(dispatch.require_ext(), name)(
      a['xq'], a['x'], a['ls'], AMP, MEAN_C, c['slope'], SHIFT, a['alpha'],
      a['kinv'], a['onehot'], *tail)
  return out.cpu() if torch.is_tensor(out) else [t.cpu() for t in out]


@pytest.mark.gpu
@pytest.mark.parametrize('weak', [False, True], ids=['strong', 'weak'])
@pytest.mark.parametrize('shape', SHAPES + [TR_SHAPE], ids=str)
def test_mean_sd_dist_against_float64(shape, weak):
  c = _case(*shape, weak, TR_ONEHOT if shape == TR_SHAPE else None)
  mean, sd, dist = _call('posterior_mean_std_linear', c)
  e_mean = float(((mean.double() - c['mean']).abs() / c['tol_mean']).max())
  e_var = float(((sd.double() ** 2 - c['var']).abs() / c['tol_var']).max())
  print(f'OBSERVED {shape} weak={weak}: error / bound {e_mean:.3f} (mean), '
        f'{e_var:.3f} (variance)')
  assert e_mean <= 1.0 and e_var <= 1.0
  assert torch.equal(dist, c['dist'])
  if shape == TR_SHAPE:
    assert int((dist > 0.3).sum()) == shape[0] // 2


@pytest.mark.gpu
@pytest.mark.parametrize('radius', [0.3, 0.0, 0.6])
@pytest.mark.parametrize('acq', ['ucb', 'lcb', 'ei', 'pi'])
@pytest.mark.parametrize('shape', SCORE_SHAPES + [TR_SHAPE], ids=str)
def test_scores_against_float64_acquisition(shape, acq, radius):
  c = _case(*shape, False, TR_ONEHOT if shape == TR_SHAPE else None)
  sd, code = c['var'].sqrt(), sc.ACQ_NAMES.index(acq)
  assert float(sd.min()) >= 0.7 * AMP
  got = _call('posterior_scores_linear', c, code, sc.COEF, MEAN_C, radius)
  out = (c['dist'] > radius) if 0.0 < radius <= 0.5 else \
      torch.zeros(shape[0], dtype=torch.bool)
  want = sc.acquisition(code, c['mean'], sd, sc.COEF, MEAN_C)
  err = (got.double() - want).abs()[~out]
  assert bool((err <= sc.acq_tolerance(code)).all())
  assert torch.equal(got[out], (-1e4 - c['dist'])[out])


@pytest.mark.gpu
@pytest.mark.parametrize('bad', ['d513', 'cpu', 'kinv', 'dtype'])
def test_bindings_reject_malformed_operands(bad):
  c = _case(3, 63, 4, False)
  if bad == 'd513':
    c = dict(c, x=torch.rand(5, 513), xq=torch.rand(2, 513),
             ls=torch.ones(513), onehot=[0] * 513, alpha=torch.rand(5),
             kinv=torch.eye(5))
  over = {'cpu': dict(xq=c['xq']), 'kinv': dict(kinv=torch.eye(62).cuda()),
          'dtype': dict(x=c['x'].double().cuda())}.get(bad, {})
  for name, tail in (('posterior_mean_std_linear', ()),
                     ('posterior_scores_linear', (0, 1.8, 0.0, 0.3))):
    with pytest.raises(RuntimeError):
      _call(name, c, *tail, **over)


def _designer(**kw):
  from vizier_amd import pyvizier as vz
  from vizier_amd._src.algorithms.core import abstractions as ab
  from vizier_amd._src.algorithms.designers import gp_bandit
  problem = vz.ProblemStatement()
  for i in range(8):
    problem.search_space.root.add_float_param(f'x{i}', 0.0, 1.0)
  problem.metric_information.append(vz.MetricInformation(
      name='obj', goal=vz.ObjectiveMetricGoal.MAXIMIZE))
  d = gp_bandit.VizierGPBandit(problem, gp_bandit.GPBanditConfig(
      linear_coef=0.4, max_evaluations=500, ard_restarts=1, ard_max_iters=10,
      **kw), seed=1)
  trials = []
  for uid, v in enumerate(np.random.default_rng(0).uniform(size=(40, 8)), 1):
    trials.append(vz.Trial({f'x{i}': float(v[i]) for i in range(8)}, id=uid))
    trials[-1].complete(vz.Measurement(
        metrics={'obj': float(v.sum() - ((v - 0.5) ** 2).sum())}))
  d.update(ab.CompletedTrials(trials), ab.ActiveTrials())
  return d


def test_unknown_linear_scorer_raises():
  with pytest.raises(ValueError, match='linear_scorer'):
    _designer(linear_scorer='bogus', device='cpu')


@pytest.mark.gpu
def test_designer_sweeps_through_the_captured_hip_scorer():
  from vizier_amd._src.ops import dispatch
  d = _designer(linear_scorer='hip', device='cuda')
  for s in d.suggest(3):
    assert all(0.0 <= v <= 1.0 for v in s.parameters.as_dict().values())
  assert d._last_optimizer.last_used_graph
  assert not d._last_optimizer.last_used_megakernel
  post, (score_fn, _) = d._posteriors[0], d._score_factory(1)
  assert post.K_inv is None and not hasattr(score_fn, 'scoring')
  dense = torch.rand(25, 8, generator=torch.Generator().manual_seed(3)).cuda()
  p, tr = post.params, d._make_trust_region()
  want = dispatch.require_ext().posterior_scores_linear(
      dense, post.x, p.lengthscales, float(p.amplitude), float(p.mean),
      0.4 * float(p.slope), 0.4 * float(p.shift), post.alpha, post.K_inv_lin,
      tr._onehot.to(torch.uint8), 0, d._config.ucb_coefficient, 0.0,
      tr.trust_radius)
  for _ in range(2):
    assert torch.equal(score_fn(d._codec.encode(dense)), want)
  t = _designer(device='cuda')     # linear_scorer='torch': today's path
  assert len(t.suggest(3)) == 3 and t._posteriors[0].K_inv_lin is None
  assert not t._last_optimizer.last_used_graph
  assert not t._last_optimizer.last_used_megakernel


def test_k_inv_lin_is_as_good_as_an_fp32_cache_can_be():
  """TestVariancePosteriorConditioning's criterion: the stored fp32 cache
  against the fp32 rounding of the float64 inverse, in float64 arithmetic."""
  g = torch.Generator().manual_seed(11)
  x, xq = torch.rand(40, 5, generator=g), torch.rand(64, 5, generator=g)
  y = x.sum(-1) + torch.sin(3.0 * x[:, 0])
  kw = dict(linear_coef=0.4, num_restarts=1, max_iters=10, seed=2)
  post = lm.train_linear_matern_gp(x, y, with_k_inv=True, **kw)
  plain = lm.train_linear_matern_gp(x, y, **kw)
  assert plain.K_inv_lin is None and plain.K_inv is None is post.K_inv
  assert post.K_inv_lin.dtype == torch.float32
  assert torch.equal(plain.alpha, post.alpha) and torch.equal(plain.L, post.L)
  p64 = lm.LinearMaternParams.from_raw(post.raw.double())
  gram = lm._combined_gram(p64, 0.4, x.double(), None)
  k = lm._combined_gram(p64, 0.4, xq.double(), x.double())
  inv = torch.linalg.inv(gram + post.noise_eff * torch.eye(40).double())
  quad = lambda m: (k * (k @ m.double())).sum(-1)
  e_stored = float((quad(post.K_inv_lin) - quad(inv)).abs().max())
  e_best = float((quad(inv.float()) - quad(inv)).abs().max())
  print(f'OBSERVED K_inv_lin: stored {e_stored:.3e}, best {e_best:.3e}')
  assert 0.0 < e_best and e_stored <= 4.0 * e_best
