"""GP-UCB-PE scorer on completed + pending rows (posterior_score_pe.hip)
against the float64 formula of its header; `PEScoringFunction` and the
`pe_scorer` knob. Operands: seeded, uniform in the unit box; lengthscales in
[0.3, 1], noise 1e-2 amp^2, W_all the float64 inverse of the (Na, Na) Gram and
W_fit that of its leading (n_fit, n_fit) block, symmetrised in float64 and
rounded to float, alpha as in scorer_cases. Asserted on the reference alone:
var and var_all >= 1e-3 amp^2. Tolerances: 4x the error of the same formula in
CPU fp32 torch plus 8 * 2^-24 of the absolute sums. Worst observed error /
bound: see the README.
"""

import functools

import pytest
import torch

import designer_cases as dc
import scorer_cases as sc

AMP, MEAN_C, U = sc.AMP, sc.MEAN_C, 2.0 ** -24
EXPLORE, PEN, RADIUS = 0.5, 10.0, 0.3
TR_ONEHOT = (0, 0, 1, 1, 1, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0)
# (b, n_fit, n_pending, d): the issue's table, row by row.
CASES = [(1, 1, 0, 1), (1, 1, 1, 1), (3, 63, 0, 4), (25, 64, 0, 3),
         (25, 63, 1, 3), (25, 64, 1, 3), (25, 65, 3, 3), (25, 128, 16, 3),
         (32, 130, 5, 5), (33, 70, 2, 4), (4, 70, 2, 64), (4, 70, 2, 65),
         (2, 70, 2, 512), (25, 1100, 3, 8)]
# Half the candidates outside RADIUS of the fitted rows; the six pending rows
# ARE six of those.
TR_CASE = (24, 70, 6, 16)
SCORE_CASES = [CASES[11], CASES[12], TR_CASE]


def _predict(c, dtype):
  """(k, mean, var, var_all) by the header's formula in `dtype`."""
  n, amp2 = c['n_fit'], torch.tensor(AMP, dtype=dtype) ** 2
  z = (c['xq'].to(dtype)[:, None, :] - c['x_all'].to(dtype)[None]) / \
      c['ls'].to(dtype)
  sr = sc.SQRT5 * (z * z).sum(-1).clamp_min(0).sqrt()
  k = amp2 * (1.0 + sr + sr * sr / 3.0) * torch.exp(-sr)
  quad = lambda kk, w: (kk * (kk @ w.to(dtype))).sum(-1)
  return (k, MEAN_C + k[:, :n] @ c['alpha'].to(dtype),
          (amp2 - quad(k[:, :n], c['w_fit'])).clamp_min(1e-12),
          (amp2 - quad(k, c['w_all'])).clamp_min(1e-12))


@functools.lru_cache(maxsize=None)
def _case(b, n, p, d):
  """Operands, float64 reference and tolerances: built once, shared."""
  g = torch.Generator().manual_seed(1000 * b + n + 31 * p + 7 * d)
  r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
  tr = (b, n, p, d) == TR_CASE
  mask = list(TR_ONEHOT) if tr else [0] * d
  x_all, xq = r(n + p, d).float(), r(b, d).float()
  if tr:
    pool = r(16 * b, d).float()
    far = sc.min_linf_dist(pool, x_all[:n], mask) > RADIUS
    xq = torch.cat([pool[~far][:b // 2], pool[far][:b - b // 2]])
    x_all[n:] = xq[b // 2:b // 2 + p]
  sign = torch.where(r(n) < 0.5, -1.0, 1.0).double()
  c = dict(xq=xq, x_all=x_all, n_fit=n, onehot=mask,
           ls=(0.3 + 0.7 * r(d)).float(),
           alpha=(sign * (0.5 + 0.5 * r(n)) / n ** 0.5).float())
  x64 = x_all.double()
  z = (x64[:, None, :] - x64[None]) / c['ls'].double()
  sr = sc.SQRT5 * (z * z).sum(-1).sqrt()
  gram = AMP ** 2 * ((1.0 + sr + sr * sr / 3.0) * torch.exp(-sr) +
                     1e-2 * torch.eye(n + p, dtype=torch.float64))
  for name, m in (('w_fit', gram[:n, :n]), ('w_all', gram)):
    inv = torch.linalg.inv(m)
    c[name] = (0.5 * (inv + inv.T)).float().contiguous()
  k, c['mean'], c['var'], c['var_all'] = _predict(c, torch.float64)
  assert float(torch.minimum(c['var'], c['var_all']).min()) >= 1e-3 * AMP ** 2
  c['dist'] = sc.min_linf_dist(xq, x_all, mask)
  if tr:  # pending rows enter the distance: six far candidates are at 0
    assert int((sc.min_linf_dist(xq, x_all[:n], mask) > RADIUS).sum()) == b // 2
    assert int((c['dist'] > RADIUS).sum()) == b // 2 - p
    assert bool((c['dist'][b // 2:b // 2 + p] == 0).all())
  _, m32, v32, a32 = _predict(c, torch.float32)
  mag = lambda kk, w: ((kk.abs() @ w.double().abs()) * kk.abs()).sum(-1)
  c['tol_mean'] = 4 * float((m32 - c['mean']).abs().max()) + \
      8 * U * (k[:, :n].abs() @ c['alpha'].double().abs())
  c['tol_var'] = 4 * float((v32 - c['var']).abs().max()) + \
      8 * U * (mag(k[:, :n], c['w_fit']) + AMP ** 2)
  c['tol_var_all'] = 4 * float((a32 - c['var_all']).abs().max()) + \
      8 * U * (mag(k, c['w_all']) + AMP ** 2)
  return c


def _call(name, c, *tail, **over):
  from vizier_amd._src.ops import dispatch
  a = dict(xq=c['xq'].cuda(), x_all=c['x_all'].cuda(), ls=c['ls'].cuda(),
           amp=AMP, mean_c=MEAN_C, alpha=c['alpha'].cuda(),
           w_fit=c['w_fit'].cuda(), w_all=c['w_all'].cuda(),
           onehot=torch.tensor(c['onehot'], dtype=torch.uint8).cuda())
  a.update(over)
  out = getattr(dispatch.require_ext(), name)(*a.values(), *tail)
  return out.cpu() if torch.is_tensor(out) else [t.cpu() for t in out]


@pytest.mark.parametrize('case', CASES + [TR_CASE], ids=str)
def test_reference_conditions_hold(case):
  c = _case(*case)
  assert c['w_all'].shape[0] == case[1] + case[2] == c['x_all'].shape[0]
  assert torch.equal(c['w_fit'], c['w_fit'].T)
  assert torch.equal(c['w_all'], c['w_all'].T)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES + [TR_CASE], ids=str)
def test_mean_sd_dist_against_float64(case):
  c = _case(*case)
  mean, sd, sd_all, dist = _call('pe_mean_std', c)
  errs = [float(((got.double() - c[ref]).abs() / c[tol]).max())
          for got, ref, tol in ((mean, 'mean', 'tol_mean'),
                                (sd ** 2, 'var', 'tol_var'),
                                (sd_all ** 2, 'var_all', 'tol_var_all'))]
  print(f'OBSERVED {case}: error / bound {errs[0]:.3f} (mean), '
        f'{errs[1]:.3f} (variance), {errs[2]:.3f} (variance, all rows)')
  assert max(errs) <= 1.0
  assert torch.equal(dist, c['dist'])
  # UCB mode (no W_all): the same mean, sd and dist, bit for bit.
  u_mean, u_sd, u_all, u_dist = _call('pe_mean_std', c, w_all=None)
  assert u_all.numel() == 0
  assert torch.equal(u_mean, mean) and torch.equal(u_sd, sd)
  assert torch.equal(u_dist, dist)


@pytest.mark.gpu
@pytest.mark.parametrize('radius', [RADIUS, 0.6])
@pytest.mark.parametrize('mode', ['ucb', 'pe'])
@pytest.mark.parametrize('case', SCORE_CASES, ids=str)
def test_scores_against_float64_acquisition(case, mode, radius):
  c = _case(*case)
  sd, sd_all = c['var'].sqrt(), c['var_all'].sqrt()
  explore = c['mean'] + EXPLORE * sd
  thr = float(explore.median())
  if mode == 'ucb':
    assert float(sd.min()) >= 0.7 * AMP  # what sc.TOL_ACQ assumes
    want, tol = c['mean'] + sc.COEF * sd, sc.acq_tolerance(0)
    got = _call('pe_scores', c, 0, sc.COEF, 0.0, 0.0, 0.0, radius, w_all=None)
  else:
    want = sd_all + PEN * (explore - thr).clamp_max(0.0)
    tol = c['tol_var_all'] / (2 * sd_all) + PEN * (
        c['tol_mean'] + EXPLORE * c['tol_var'] / (2 * sd))
    got = _call('pe_scores', c, 1, 0.0, EXPLORE, thr, PEN, radius)
  out = (c['dist'] > radius) if radius <= 0.5 else \
      torch.zeros(case[0], dtype=torch.bool)
  ratio = ((got.double() - want).abs() / tol)[~out]
  if ratio.numel():
    print(f'OBSERVED {case} {mode}: error / bound {float(ratio.max()):.3f}')
  assert bool((ratio <= 1.0).all())
  assert torch.equal(got[out], (-1e4 - c['dist'])[out])
  if case == TR_CASE and radius == RADIUS:
    assert int(out.sum()) == case[0] // 2 - case[2]


@pytest.mark.gpu
@pytest.mark.parametrize('bad', ['noncontig', 'dtype', 'cpu', 'nfit', 'wfit',
                                 'wall', 'd513', 'n4096'])
def test_bindings_reject_malformed_operands(bad):
  c = _case(3, 63, 0, 4)
  z = lambda *s: torch.zeros(*s, device='cuda')
  over = {
      'noncontig': dict(xq=z(4, 3).T),
      'dtype': dict(x_all=c['x_all'].double().cuda()),
      'cpu': dict(alpha=c['alpha']),
      'nfit': dict(alpha=z(64), w_fit=z(64, 64)),
      'wfit': dict(w_fit=z(63, 62)),
      'wall': dict(w_all=z(62, 62)),
      'd513': dict(xq=z(2, 513), x_all=z(63, 513), ls=z(513) + 1,
                   onehot=z(513).to(torch.uint8)),
      'n4096': dict(x_all=z(4096, 4), w_all=z(1, 1))}[bad]
  for name, tail in (('pe_mean_std', ()),
                     ('pe_scores', (1, 0.0, EXPLORE, 0.0, PEN, RADIUS))):
    with pytest.raises(RuntimeError):
      _call(name, c, *tail, **over)


def test_unknown_value_and_hip_on_cpu_raise():
  with pytest.raises(ValueError, match='pe_scorer'):
    dc.ucbpe_setup('float', 1, 0, 'cpu', pe_scorer='bogus')
  s = dc.ucbpe_setup('float', 1, 0, 'cpu', pe_scorer='hip')
  for use_ucb in (True, False):
    with pytest.raises(ValueError, match='GPU device'):
      s.designer._one_score_fn(use_ucb, s.x_all)


@pytest.mark.parametrize('row,safe', [
    ('ucb-mixed', None), ('ucb-mixed-pending', False), ('pe-mixed', False),
    ('pe-mixed-pending', False)])
def test_default_keeps_todays_closures(row, safe):
  setup, _, use_ucb = dc.ucbpe_case(row, True, 'cpu')
  assert setup.designer._config.pe_scorer == 'torch'
  score_fn = setup.designer._one_score_fn(use_ucb, setup.x_all)
  assert getattr(score_fn, 'graph_safe', None) is safe
  assert hasattr(score_fn, 'scoring') == (safe is None)


@pytest.mark.gpu
def test_designer_scores_and_sweeps_through_the_hip_scorer(monkeypatch):
  setup = dc.ucbpe_setup('mixed', 1, 2, 'cuda', pe_scorer='hip',
                         max_evaluations=2000)
  d, x_all = setup.designer, setup.x_all
  cands = dc.make_candidates('mixed', x_all)
  t = dc.ucbpe_case('ucb-mixed-pending', True, 'cuda')[0]  # pe_scorer='torch'
  assert t.designer._one_score_fn(True, t.x_all).graph_safe is False
  for use_ucb in (True, False):
    score_fn = d._one_score_fn(use_ucb, x_all)
    assert score_fn.graph_safe is True and not hasattr(score_fn, 'scoring')
    want = dc.ucbpe_oracle(setup, cands, use_ucb)
    assert int(want.penalised.sum()) == dc.B // 2
    got = score_fn(cands.batch('cuda')).cpu().double()
    assert bool(((got - want.value).abs() <= want.tol).all())
    # The captured sweep ends on the eager sweep's candidate, bit for bit.
    captured = d._optimize_one(use_ucb, x_all)
    assert d._last_optimizer.last_used_graph is True
    with monkeypatch.context() as m:
      def eager_fn(batch, fn=score_fn):
        return fn(batch)
      eager_fn.graph_safe = False
      m.setattr(d, '_one_score_fn', lambda *_: eager_fn)
      eager = d._optimize_one(use_ucb, x_all)
      assert d._last_optimizer.last_used_graph is False
    assert torch.equal(captured, eager)
  used, one = [], d._optimize_one
  def counted(*args):
    out = one(*args)
    used.append(d._last_optimizer.last_used_graph)
    return out
  monkeypatch.setattr(d, '_optimize_one', counted)
  assert len(d.suggest(3)) == 3 and used == [True] * 3
