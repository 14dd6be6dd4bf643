"""CPU self-check of tests/scorer_cases.py (no GPU needed).

Proves that the reference alone sits well inside every bound that
tests/test_scorer_branches.py asserts on the GPU, and that no case is
degenerate: for every shape, an fp32 torch emulation of the reference
formulas agrees with fp64 to within one eighth of the bound.
"""

import pytest
import torch

import scorer_cases as sc


def _ids(shapes):
  return ['-'.join(str(v) for v in s) for s in shapes]


@pytest.mark.parametrize('b,n,d', sc.ALL_DENSE_SHAPES,
                         ids=_ids(sc.ALL_DENSE_SHAPES))
def test_dense_case_is_well_conditioned(b, n, d):
  case = sc.dense_case(b, n, d)
  for t in (case.x, case.xq, case.ls, case.alpha, case.M):
    assert t.dtype == torch.float32 and not t.is_cuda
  assert not torch.equal(case.M, case.M.T)
  ref = sc.dense_reference(b, n, d)
  emu = sc.reference(case, dtype=torch.float32)
  assert float(ref.k.min()) / sc.AMP2 >= 0.5
  assert float(ref.sd.min()) >= 0.5 * sc.AMP
  assert abs(float(ref.quad.max()) - 0.5 * sc.AMP2) < 1e-6
  e_mean = float((emu.mean.double() - ref.mean).abs().max())
  e_quad = float((emu.quad.double() - ref.quad).abs().max())
  assert e_mean <= sc.TOL_FP32 / 8, e_mean
  assert e_quad <= sc.TOL_FP32 / 8, e_quad
  # The same for what the GPU tests read back: quad = amp^2 - sd^2.
  sd32 = emu.sd.double()
  assert float(((sc.AMP2_F32 - sd32 * sd32) - ref.quad).abs().max()) <= (
      sc.TOL_FP32 / 8)


@pytest.mark.parametrize('b,n,d', sc.ACQ_SHAPES, ids=_ids(sc.ACQ_SHAPES))
def test_acquisition_forms(b, n, d):
  ref = sc.dense_reference(b, n, d)
  emu = sc.reference(sc.dense_case(b, n, d), dtype=torch.float32)
  best = float(ref.mean.median())
  z = (ref.mean - best) / ref.sd
  assert float(z.min()) < 0 < float(z.max())
  for code in range(6):
    want = sc.acquisition(code, ref.mean, ref.sd, sc.COEF, best)
    got = sc.acquisition(code, emu.mean, emu.sd, sc.COEF, best)
    assert got.dtype == torch.float32
    err = float((got.double() - want).abs().max())
    assert err <= sc.acq_tolerance(code) / 8, (code, err)
  # PI and EI against closed forms that do not go through erfc.
  normal = torch.distributions.Normal(0.0, 1.0)
  pi = sc.acquisition(3, ref.mean, ref.sd, sc.COEF, best)
  assert float((pi - normal.cdf(z)).abs().max()) < 1e-12
  ei = sc.acquisition(2, ref.mean, ref.sd, sc.COEF, best)
  want = ref.sd * (z * normal.cdf(z) + normal.log_prob(z).exp())
  assert float((ei - want).abs().max()) < 1e-12


@pytest.mark.parametrize('kind', ['bf16', 'fp8'])
@pytest.mark.parametrize('b,n,d', sc.ALL_DENSE_SHAPES,
                         ids=_ids(sc.ALL_DENSE_SHAPES))
def test_lowp_reference(kind, b, n, d):
  """The rounded-operand reference: operands from the production code,
  emulation error far below the floor of the bound, and the rounding
  itself visible (so the plain fp64 reference would NOT do)."""
  case = sc.dense_case(b, n, d)
  lo = sc.Operands(case, 'cpu').lowp_operands(kind)
  dp = (d + 31) // 32 * 32
  assert lo['z1'].shape == (b, dp) and lo['z2'].shape == (n, dp)
  assert lo['n2'].shape == (n,)
  ref, tol_m, tol_q, (e_mean, e_quad) = sc.lowp_bounds(case, lo)
  assert e_mean <= sc.TOL_FP32 / 8 and e_quad <= sc.TOL_FP32 / 8
  assert tol_m == sc.TOL_FP32 and tol_q == sc.TOL_FP32
  assert float(ref.sd.min()) >= 0.5 * sc.AMP
  plain = sc.dense_reference(b, n, d)
  # bf16 keeps 8 bits, e4m3 keeps 4: k moves by far more than fp32 noise
  # but the case stays the same case.
  moved = float((ref.k - plain.k).abs().max()) / sc.AMP2
  assert 1e-6 < moved < 0.1, moved


@pytest.mark.parametrize('branch,b,n,nearest', sc.TR_CASES,
                         ids=_ids(sc.TR_CASES))
def test_trust_region_case(branch, b, n, nearest):
  case = sc.tr_case(b, n, nearest)
  ref = sc.reference(case, sc.TR_ONEHOT)
  emu = sc.reference(case, sc.TR_ONEHOT, dtype=torch.float32)
  h = b // 2
  assert float((ref.dist - sc.TR_RADIUS).abs().min()) >= 0.05
  assert float((ref.dist[:h] - sc.TR_NEAR).abs().max()) < 1e-6
  assert float((ref.dist[h:] - sc.TR_FAR).abs().max()) < 1e-6
  # The mirror image under the inverted mask; the nearest row is unique.
  flipped = sc.min_linf_dist(case.xq.double(), case.x.double(),
                             [1 - v for v in sc.TR_ONEHOT])
  assert float((flipped[:h] - sc.TR_FAR).abs().max()) < 1e-6
  assert float((flipped[h:] - sc.TR_NEAR).abs().max()) < 1e-6
  keep = ~torch.tensor(sc.TR_ONEHOT, dtype=torch.bool)
  per_row = (case.xq[:, None] - case.x)[..., keep].abs().amax(-1)
  assert bool((per_row.argmin(-1) == nearest).all())
  assert float(ref.sd.min()) >= 0.5 * sc.AMP
  ucb = sc.acquisition(0, ref.mean, ref.sd, sc.COEF, 0.0)
  got = sc.acquisition(0, emu.mean, emu.sd, sc.COEF, 0.0).double()
  assert float((got - ucb).abs().max()) <= sc.TOL_ACQ / 8


@pytest.mark.parametrize('path,b,n,d',
                         sc.SPIKE_SHAPES + [('custom', 25, 4100, 8)])
def test_spike_pairs(path, b, n, d):
  pairs = sc.spike_pairs(b, n, path)
  assert len(set(pairs)) == len(pairs)
  assert all(0 <= i < n and 0 <= j < n for i, j in pairs)
  rows = {i for i, _ in pairs}
  assert {0, n - 1, n // 2, n // 10, n // 10 - 1, 9 * n // 10} <= rows
  assert (0, n - 1) in pairs and (n - 1, 0) in pairs
  if path in ('split', 'custom'):
    rchunks = 512 // b
    assert {n // rchunks, (rchunks - 1) * n // rchunks - 1} <= rows
  if path == 'custom':
    assert {256, 255, 4096, 4095} <= rows
  # An exact spike evaluated in fp64 has zero error by construction.
  k = sc.dense_reference(b, n, d).k
  i = torch.tensor([p[0] for p in pairs])
  j = torch.tensor([p[1] for p in pairs])
  means = sc.MEAN_C + k[:, i].T
  sds = (sc.AMP2_F32 - sc.SPIKE_C * k[:, i].T * k[:, j].T).sqrt()
  e_mu, e_q = sc.spike_errors(k, pairs, means, sds)
  assert float(e_mu.max()) < 1e-12 and float(e_q.max()) < 1e-12
