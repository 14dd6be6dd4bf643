"""CPU conditions on tests/gram_cases.py: the inputs exercise the kernels, the
exact family is exact, the CPU fp32 reference meets the derived bound, and
the bound is tight enough to see the MFMA bindings' norm contract.

Everything the GPU file (tests/test_gram_kernels.py) compares against is
checked here first, without a GPU.
"""

import pytest
import torch

import gram_cases as gc


def fp32_cases():
  return [gc.make_case(n, m, d) for d in gc.FP32_D
          for n, m in gc.FP32_SHAPES]


def sym_cases():
  return [gc.make_case(n, n, d, sym=True) for d in gc.SYM_D
          for n in gc.SYM_N]


def mfma_shapes():
  return [(n, m, d) for d in gc.STRIP_D for n, m in gc.strip_shapes()] + \
      [(n, m, d) for d in gc.TILED_D for n, m in gc.TILED_SHAPES]


def exact_shapes():
  return [(17, 33, 33), (33, 65, 65), (128, 64, 31), (129, 127, 90)]


def rounded(case, kind):
  """(q1, q2, scale) of a case on the CPU."""
  if kind == 'bf16':
    return gc.bf16_operands(case.x1, case.x2, case.ls) + (1.0,)
  return gc.fp8_operands(case.x1, case.x2, case.ls)


# -- the inputs make the check bite ----------------------------------------------


def check_value_range(name, k, amp):
  """The two conditions of the module docstring on one fp64 reference."""
  rel = k / amp ** 2
  if k.numel() >= 64:
    inside = float(((rel >= 0.05) & (rel <= 0.95)).double().mean())
    assert inside >= 0.5, (name, inside)
    assert float(rel.min()) < 1e-6, (name, float(rel.min()))


def test_value_range_fp32_cases():
  for case in fp32_cases() + sym_cases():
    check_value_range(case.name, gc.oracle_fp32(case), case.amp)


def test_value_range_batched_cases():
  """Restart 0 (unit lengthscale factor, no far row lost) holds the
  conditions; K - noise I is what is looked at."""
  for d in gc.BATCHED_D:
    for n in gc.BATCHED_N:
      case = gc.make_case(n, n, d, sym=True)
      ls, amp, noise = gc.batched_params(case, 3)
      K, _ = gc.oracle_batched(case, ls, amp, noise)
      K0 = K[0] - float(noise[0]) * torch.eye(n, dtype=torch.float64)
      check_value_range(case.name, K0, float(amp[0]))


@pytest.mark.parametrize('kind', ['bf16', 'fp8'])
def test_value_range_mfma_cases(kind):
  for n, m, d in mfma_shapes():
    case = gc.make_case(n, m, d)
    q1, q2, s = rounded(case, kind)
    check_value_range(case.name, gc.mfma_oracle(q1, q2, case.amp, s).k,
                      case.amp)


def test_planted_rows_are_what_they_claim():
  """dup: d^2 = 0; near: 0 < sqrt5 r < 0.1; far: sqrt5 r in [15, 30]."""
  seen = set()
  for case in fp32_cases() + sym_cases():
    s = (5.0 * gc.diff_d2(case.x1, case.x2, case.ls)).sqrt()
    for kind, i, j in case.planted:
      seen.add(kind)
      v = float(s[i, j])
      if kind == 'dup':
        assert v == 0.0, (case.name, i, j, v)
      elif kind == 'near':
        assert 0.0 < v < 0.1, (case.name, i, j, v)
      else:
        assert 15.0 <= v <= 30.0, (case.name, i, j, v)
  assert seen == {'dup', 'near', 'far'}


# -- the exact-operand family ------------------------------------------------------


@pytest.mark.parametrize('kind,levels', [('bf16', 32), ('fp8', 8)])
def test_exact_family_rounding_is_a_no_op(kind, levels):
  """The rounded-operand oracle equals plain gram_matern52 on the unrounded
  inputs to 1e-14 amp^2, the rounding itself changes no bit, d^2 is an
  integer multiple of 4^-p below 2^24, and coincident rows give exactly
  amp^2."""
  for n, m, d in exact_shapes():
    case = gc.make_exact_case(n, m, d, levels)
    q1, q2, s = rounded(case, kind)
    z1 = case.x1 / case.ls
    assert torch.equal(q1[:, :d].float() * s, z1), case.name
    assert torch.equal(q2[:, :d].float() * s, case.x2 / case.ls), case.name
    ref = gc.mfma_oracle(q1, q2, case.amp, s, exact=True)
    plain = gc.oracle_fp32(case)
    assert float((ref.k - plain).abs().max()) <= 1e-14 * case.amp ** 2, \
        case.name
    quantum = (float(z1.max()) / levels) ** 2     # 4^-p: z1[0, 0] = levels 2^-p
    units = ref.d2 / quantum
    assert float(units.max()) < 2 ** 24
    assert float((units - units.round()).abs().max()) < 1e-6, case.name
    assert case.planted
    for _, i, j in case.planted:
      assert float(ref.k[i, j]) == case.amp ** 2


def test_exact_family_fp32_reference_has_exact_d2():
  """In the exact family the fp32 difference form is exact too: the CPU
  fp32 reference differs from fp64 by the epilogue alone."""
  for n, m, d in exact_shapes():
    for levels in (8, 32):
      case = gc.make_exact_case(n, m, d, levels)
      d2 = gc._diff_d2_fp32(case.x1, case.x2, case.ls)
      assert torch.equal(d2.double(),
                         gc.diff_d2(case.x1, case.x2, case.ls)), case.name
      ratio = gc.worst_ratio(gc.reference_fp32(case), gc.oracle_fp32(case),
                             gc.bound_fp32(case))
      assert ratio < 1.0, (case.name, ratio)


# -- the CPU fp32 reference stays inside the derived bound ----------------------------


def test_fp32_reference_within_bound():
  worst = 0.0
  for case in fp32_cases() + sym_cases():
    ratio = gc.worst_ratio(gc.reference_fp32(case), gc.oracle_fp32(case),
                           gc.bound_fp32(case))
    assert ratio < 1.0, (case.name, ratio)
    worst = max(worst, ratio)
  print(f'OBSERVED fp32 gram: CPU fp32 reference worst {worst:.4f} of the '
        'bound')
  assert worst > 0.01          # the bound is no formality


def test_batched_reference_within_bound():
  worst = [0.0, 0.0]
  for d in gc.BATCHED_D:
    for n in gc.BATCHED_N:
      case = gc.make_case(n, n, d, sym=True)
      for r in gc.BATCHED_R:
        params = gc.batched_params(case, r)
        got = gc.reference_batched(case, *params)
        want = gc.oracle_batched(case, *params)
        bound = gc.bound_batched(case, *params)
        for i in range(2):
          ratio = gc.worst_ratio(got[i], want[i], bound[i])
          assert ratio < 1.0, (case.name, r, 'KG'[i], ratio)
          worst[i] = max(worst[i], ratio)
  print(f'OBSERVED batched gram: CPU fp32 reference worst K {worst[0]:.4f} '
        f'G {worst[1]:.4f} of the bound')
  assert min(worst) > 0.01


@pytest.mark.parametrize('kind', ['bf16', 'fp8'])
def test_mfma_reference_within_bound(kind):
  worst = 0.0
  for n, m, d in mfma_shapes():
    case = gc.make_case(n, m, d)
    q1, q2, s = rounded(case, kind)
    ref = gc.mfma_oracle(q1, q2, case.amp, s)
    ratio = gc.worst_ratio(gc.mfma_reference_fp32(q1, q2, case.amp, s),
                           ref.k, ref.bound)
    assert ratio < 1.0, (case.name, ratio)
    worst = max(worst, ratio)
  print(f'OBSERVED {kind} gram: CPU fp32 reference worst {worst:.4f} of the '
        'bound')
  assert worst > 0.01


@pytest.mark.parametrize('kind,levels', [('bf16', 32), ('fp8', 8)])
def test_mfma_reference_within_exact_bound(kind, levels):
  for n, m, d in exact_shapes():
    case = gc.make_exact_case(n, m, d, levels)
    q1, q2, s = rounded(case, kind)
    ref = gc.mfma_oracle(q1, q2, case.amp, s, exact=True)
    ratio = gc.worst_ratio(gc.mfma_reference_fp32(q1, q2, case.amp, s),
                           ref.k, ref.bound)
    assert ratio < 1.0, (case.name, ratio)


# -- the bound sees the contracts ---------------------------------------------------


def test_bound_sees_norms_of_unrounded_operands():
  """bf16 contract: d^2 is the exact squared distance of the ROUNDED
  vectors. An oracle with the norms of the unrounded z (what a binding that
  took its norms before rounding would compute) must leave the bound, in
  every case with more than a handful of entries."""
  for n, m, d in mfma_shapes():
    case = gc.make_case(n, m, d)
    if n * m < 64:
      continue
    q1, q2, _ = rounded(case, 'bf16')
    right = gc.mfma_oracle(q1, q2, case.amp)
    z1, z2 = case.x1 / case.ls, case.x2 / case.ls
    wrong = gc.mfma_oracle(q1, q2, case.amp,
                           n1=(z1.double() ** 2).sum(-1),
                           n2=(z2.double() ** 2).sum(-1))
    ratio = gc.worst_ratio(wrong.k, right.k, right.bound)
    assert ratio > 1.0, (case.name, ratio)


def test_bound_sees_a_transposed_or_shifted_result():
  """A transposed square cross-gram and a result shifted by one column
  leave the bound (what a wrong swizzle or fragment layout produces)."""
  case = gc.make_case(17, 17, 33)
  q1, q2, _ = rounded(case, 'bf16')
  ref = gc.mfma_oracle(q1, q2, case.amp)
  assert gc.worst_ratio(ref.k.T, ref.k, ref.bound) > 1.0
  assert gc.worst_ratio(ref.k.roll(1, 1), ref.k, ref.bound) > 1.0


def test_bound_sees_a_missing_fp8_scale():
  """fp8 contract: the dot is multiplied back by scale^2."""
  case = gc.make_case(17, 33, 33)
  q1, q2, s = rounded(case, 'fp8')
  ref = gc.mfma_oracle(q1, q2, case.amp, s)
  z1, z2 = q1.float().double(), q2.float().double()
  n1, n2 = (z1 * z1).sum(-1) * s * s, (z2 * z2).sum(-1) * s * s
  d2 = (n1[:, None] + n2[None, :] - 2.0 * (z1 @ z2.mT)).clamp_min(0.0)
  assert gc.worst_ratio(case.amp ** 2 * gc.k_of_d2(d2), ref.k,
                        ref.bound) > 1.0
