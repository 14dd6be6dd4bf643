"""The scorers the designers hand to the sweep, against fp64 oracles (GPU).

Every kernel is held to an fp64 oracle on synthetic operands elsewhere. Here
the closure the DESIGNER returns is called: VizierGPUCBPEBandit._one_score_fn
(UCB and PE, one and two metrics, with and without pending trials, plain and
linear kernel) and the multi-objective closure of
VizierGPBandit._score_factory (fp32, fp8, bf16 candidate grams). Each test
asserts which path engaged and compares the values with the oracle of
tests/designer_cases.py, which writes each score from its formula on the
designer's own stored operands: a wrong posterior, K^-1, threshold, mask,
radius or distance anchor moves a score by 100x the bound or more
(tests/test_designer_cases.py; swapped metrics in the float space with the
region on move it 5.5x only, see SWAP_FLOOR there), a wrong cache (the PE variance posterior)
fails tests/test_gp_ucb_pe.py.

Cases, oracle and the derivation of the bounds: tests/designer_cases.py.
`pytest -rA` prints one OBSERVED line per test: the largest error over its
bound among the candidates inside the trust radius (compared by value) and
among those outside (-1e4 - dist, bound scorer_cases.TOL_PENALTY).

Observed on the MI355X, largest error (and the smallest .. largest bound
among the candidates it was taken over); the same with the region off:
  ucb-float 1.5e-05 (2.1e-02 .. 1.1e-01)   ucb-mixed 2.2e-06 (7.1e-05 ..
  1.4e-02)   ucb-mixed-pending 4.8e-07   pe-mixed 6.6e-06 (3.6e-05 ..
  2.6e-02)   pe-mixed-pending 7.7e-06   pe-linear-pending 2.7e-05 (6.1e-05
  .. 8.1e-02)   mo-ucb-float 1.3e-05   mo-ucb-mixed 1.9e-06 (7.7e-05 ..
  3.4e-02)   mo-ucb-mixed-pending 2.1e-06   mo-pe-mixed-pending 1.7e-05
  (7.5e-05 .. 1.5e-01)   bandit fp32 1.9e-06, fp8 8.0e-06 (7.5e-05 ..
  4.0e-04), bf16 1.2e-05 (6.4e-05 .. 1.5e-04)
  largest error over bound: fp32 rows 0.005, fp8 0.038, bf16 0.080; outside
  the radius 0.24 (half an fp32 ulp at 1e4 against 2e-3).
The fp32 bounds are loose next to the data: they carry the coherent worst
case of sum |k||K^-1||k|, which at noise 1e-2 amp^2 is several hundred amp^2.
"""

import pytest
import torch

import designer_cases as dc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
LEGS = [True, False]
LEG_IDS = ['tr', 'no-tr']

# What must engage, per row of dc.UCBPE_ROWS, with the trust region on:
#   'hip'    score_fn.scoring (the pure-HIP chunked scorer, megakernel
#            eligible), anchored; 'fused': graph_safe is True; 'eager':
#            graph_safe is False.
UCBPE_PATHS = {
    'ucb-float': 'hip', 'ucb-mixed': 'hip', 'ucb-mixed-pending': 'eager',
    'pe-mixed': 'fused', 'pe-mixed-pending': 'fused',
    'pe-linear-pending': 'eager',
    'mo-ucb-float': 'fused', 'mo-ucb-mixed': 'fused',
    'mo-ucb-mixed-pending': 'eager', 'mo-pe-mixed-pending': 'fused',
}
BANDIT_PATHS = {'fp32': 'fused', 'fp8': 'fused', 'bf16': 'eager'}


@pytest.fixture(scope='module')
def ext():
  from vizier_amd._src.ops import dispatch
  return dispatch.require_ext()  # Fails loudly if the .so is missing.


def _expected_path(row: str, trust_region: bool) -> str:
  # Without a trust region nothing anchors on x_all, so the single-metric
  # UCB scorer is the pure-HIP one even with pending trials.
  if row == 'ucb-mixed-pending' and not trust_region:
    return 'hip'
  return UCBPE_PATHS[row]


def _assert_path(score_fn, path: str, codec=None):
  if path == 'hip':
    assert score_fn.scoring._tr_anchored is True
    assert score_fn.scoring._acq_name == 'ucb'
    assert score_fn.codec_identity == codec.identity
    assert not hasattr(score_fn, 'graph_safe')
  else:
    assert not hasattr(score_fn, 'scoring')
    assert score_fn.graph_safe is (path == 'fused')


def _compare(name: str, got: torch.Tensor, want: dc.Scored):
  got = got.detach().cpu().double()
  assert got.shape == want.value.shape
  assert bool(torch.isfinite(got).all())
  ratio = (got - want.value).abs() / want.tol
  inside, outside = ~want.penalised, want.penalised
  err = (got - want.value).abs()
  line = (f'OBSERVED {name}: inside {float(ratio[inside].max()):.3f} of the '
          f'bound (error {float(err[inside].max()):.2e}, bounds '
          f'{float(want.tol[inside].min()):.1e} .. '
          f'{float(want.tol[inside].max()):.1e})')
  if bool(outside.any()):
    line += (f', outside {float(ratio[outside].max()):.3f} '
             f'({int(outside.sum())} of {got.numel()}, radius '
             f'{want.radius:.3f})')
  print(line)
  assert bool((ratio <= 1.0).all()), (name, ratio)


def _count_calls(ext, monkeypatch, names):
  """Wraps the named bindings of the extension; returns the live counts."""
  calls = {name: 0 for name in names}
  for name in names:
    def counted(*args, _name=name, _fn=getattr(ext, name)):
      calls[_name] += 1
      return _fn(*args)
    monkeypatch.setattr(ext, name, counted)
  return calls


@pytest.mark.parametrize('trust_region', LEGS, ids=LEG_IDS)
@pytest.mark.parametrize('row', [r[0] for r in dc.UCBPE_ROWS])
def test_ucbpe_score_fn(ext, monkeypatch, row, trust_region):
  setup, cands, use_ucb = dc.ucbpe_case(row, trust_region, DEV)
  d = setup.designer
  assert setup.x_all.is_cuda and d._posterior.x.shape[0] == dc.N_DONE
  assert setup.x_all.shape[0] == dc.N_DONE + setup.n_pending
  score_fn = d._one_score_fn(use_ucb, setup.x_all)
  _assert_path(score_fn, _expected_path(row, trust_region), d._codec)
  if row == 'mo-ucb-mixed-pending':
    # Why it is eager: the posteriors are not anchored on x_all.
    assert d._fusable(d._mo_posteriors[0])
    assert not d._fusable(d._mo_posteriors[0], setup.x_all)
  if row == 'pe-linear-pending':
    assert not d._fusable(d._posterior)
  want = dc.ucbpe_oracle(setup, cands, use_ucb)
  if trust_region:
    assert int(want.penalised.sum()) == dc.B // 2
  else:
    assert want.dist is None and not bool(want.penalised.any())
  calls = _count_calls(ext, monkeypatch,
                       ['posterior_scores_chunked', 'posterior_mean_std'])
  got = score_fn(cands.batch(DEV))
  path = _expected_path(row, trust_region)
  n_metrics = 1 if d._mo_posteriors is None else 2
  if path == 'hip':
    # The pure-HIP scorer itself ran, not a composed path inside
    # ScoringFunction.__call__.
    assert calls == {'posterior_scores_chunked': 1, 'posterior_mean_std': 0}
  elif path == 'fused':
    # One (mean, sd, dist) call per posterior, and per variance posterior.
    assert calls == {'posterior_scores_chunked': 0,
                     'posterior_mean_std': n_metrics * (1 if use_ucb else 2)}
  else:
    assert calls == {'posterior_scores_chunked': 0, 'posterior_mean_std': 0}
  _compare(f'{row} {"tr" if trust_region else "no-tr"}', got, want)


@pytest.mark.parametrize('trust_region', LEGS, ids=LEG_IDS)
@pytest.mark.parametrize('gram_dtype', [r[1] for r in dc.BANDIT_ROWS])
def test_bandit_mo_score_fn(ext, monkeypatch, gram_dtype, trust_region):
  setup, cands = dc.bandit_case(gram_dtype, trust_region, DEV)
  d = setup.designer
  calls = _count_calls(ext, monkeypatch, [
      'posterior_mean_std', 'posterior_mean_std_fp8', 'gram_matern52_bf16'])
  score_fn, n_parallel = d._score_factory(1)
  assert n_parallel == 1
  _assert_path(score_fn, BANDIT_PATHS[gram_dtype])
  want = dc.bandit_oracle(setup, cands)
  got = score_fn(cands.batch(DEV))
  # One call per metric, of the binding the configured dtype names.
  used = {'fp32': 'posterior_mean_std', 'fp8': 'posterior_mean_std_fp8',
          'bf16': 'gram_matern52_bf16'}[gram_dtype]
  assert calls == {name: (2 if name == used else 0) for name in calls}
  name = f'bandit-mo-{gram_dtype} {"tr" if trust_region else "no-tr"}'
  if gram_dtype != 'fp32':
    emu = want.info['emulation']
    print(f'  {name}: fp32 emulation errors (mean, quad) per metric '
          f'{[tuple(f"{v:.1e}" for v in e) for e in emu]}')
  _compare(name, got, want)
