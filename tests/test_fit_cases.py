"""CPU conditions on tests/fit_cases.py: the oracle is right, fp32 can factor
every case, the CPU fp32 product path meets the stagewise bounds, and the
bounds see the slips they are there for.

Everything the GPU file (tests/test_fit_kernels.py) compares against is
checked here first, without a GPU.
"""

import math

import pytest
import torch

import fit_cases as fc
from vizier_amd._src.gp import gp_model

GROUP_IDS = [f'd{d}-noise{noise_rel:g}' for d, noise_rel in fc.GROUPS]


def failing_row_cases():
  return [fc.nan_case(n) for n in fc.NAN_N] + \
      [fc.make_dup_case(n) for n in fc.DUP_N]


def gate_cases():
  return [fc.make_gate_case(n) for n in (97, 1024, 1025, 1200, 1201)] + \
      [fc.make_gate_case(97, 1)]


def cpu_stages(case):
  """(nll, L, info, z (r, n)) of the CPU fp32 product path."""
  nll, L, info, z = gp_model.nll_values_with_chol_z(case.raw, case.x, case.y)
  return nll, L, info, z.squeeze(-1)


def test_cases_are_what_they_claim():
  """Distinct parameters per restart at the stated noise ratio, and raw is
  the inverse of from_raw to fp32 rounding."""
  for case in fc.all_fit_cases():
    assert case.raw.shape == (3, case.d + 3) and case.raw.dtype == torch.float32
    p = gp_model.GPParams.from_raw(case.raw.double())
    noise_rel = float(case.name.split('noise')[1].split('-')[0])
    assert torch.allclose(p.noise / p.amplitude ** 2,
                          torch.full((3,), noise_rel, dtype=torch.float64),
                          rtol=1e-4), case.name
    assert bool(((p.amplitude >= 0.5) & (p.amplitude <= 1.5)).all())
    assert bool((p.mean.abs() <= 0.2 + 1e-6).all())
    lo, hi = 0.42 * math.sqrt(case.d), 0.84 * math.sqrt(case.d)
    assert bool(((p.lengthscales >= lo * (1 - 1e-5)) &
                 (p.lengthscales <= hi * (1 + 1e-5))).all())
    for a, b in ((0, 1), (0, 2), (1, 2)):
      assert float((p.lengthscales[a] - p.lengthscales[b]).abs().min()) > 0
      assert float((p.mean[a] - p.mean[b]).abs()) > 1e-4, case.name
      assert float((p.amplitude[a] - p.amplitude[b]).abs()) > 1e-4, case.name
  for n in fc.DUP_N:
    case = fc.make_dup_case(n)
    for i in range(fc.DUP_PAIRS):
      assert torch.equal(case.x[i], case.x[n - 1 - i])
    noise = gp_model.GPParams.from_raw(case.raw.double()).noise
    assert float(noise[1]) < 1.0001e-10
  for n in fc.NAN_N:
    case, base = fc.nan_case(n), fc.make_fit_case(n, *fc.NAN_GROUP)
    assert math.isnan(float(case.raw[1, 0]))
    assert torch.equal(case.raw[[0, 2]], base.raw[[0, 2]])


@pytest.mark.parametrize('group', fc.GROUPS, ids=GROUP_IDS)
def test_fp64_analytic_gradient_matches_autograd(group):
  """The trace identities in fp64 against the autograd oracle, rtol 1e-9
  (of the largest component per restart for the gradient)."""
  for case in fc.group_cases(*group):
    nll64, grad64 = fc.oracle(case)
    nll, grad = gp_model.nll_value_and_grad(
        case.raw.double(), case.x.double(), case.y.double())
    assert bool(torch.isfinite(nll64).all()), case.name
    assert torch.allclose(nll, nll64, rtol=1e-9, atol=0.0), case.name
    err = fc.grad_error(grad, grad64)
    assert float(err.max()) <= 1e-9, (case.name, err.tolist())


@pytest.mark.parametrize('group', fc.GROUPS, ids=GROUP_IDS)
def test_cpu_fp32_factors_and_meets_the_stage_bounds(group):
  """CPU fp32 cholesky_ex gives info == 0 on every case, and the CPU fp32
  product path stays below 1.0 of the L, z and NLL stage bounds."""
  worst = 0.0
  for case in fc.group_cases(*group):
    nll, L, info, z = cpu_stages(case)
    assert info.tolist() == [0, 0, 0], case.name
    p = gp_model.GPParams.from_raw(case.raw)
    for r in range(3):
      assert fc.solve_ratio(L[r], z[r], case.y, p.mean[r]) <= 1.0, case.name
      ratio = fc.nll_ratio(nll[r], L[r], z[r], case.raw[r])
      assert ratio < 1.0, (case.name, r, ratio)
      worst = max(worst, ratio)
  print(f'OBSERVED {group}: CPU fp32 product path worst {worst:.4f} of the '
        'NLL stage bound')


def test_cpu_group_worsts_are_finite():
  """What the GPU is held to 4x of: finite and above fp32 resolution of the
  oracle (a zero would make the criterion unpassable by luck)."""
  for group, gid in zip(fc.GROUPS, GROUP_IDS):
    gw, nw = fc.cpu_group_worst(*group)
    print(f'OBSERVED {gid}: CPU fp32 worst grad {gw:.3e} nll {nw:.3e}')
    assert fc.U < gw < 1e-1 and fc.U / 4 < nw < 1e-1, (gid, gw, nw)
  gw, nw = fc.cpu_dup_worst()
  print(f'OBSERVED dup: CPU fp32 worst grad {gw:.3e} nll {nw:.3e}')
  assert fc.U < gw < 1e-1 and fc.U / 4 < nw < 1e-1


def test_failing_row_cases_have_a_finite_oracle_on_healthy_rows():
  for case in failing_row_cases():
    assert case.healthy == (0, 2)
    nll64, grad64 = fc.oracle(case)
    assert nll64.shape == (2,) and grad64.shape == (2, case.d + 3)
    assert bool(torch.isfinite(nll64).all()), case.name
    assert bool(torch.isfinite(grad64).all()), case.name
    assert float(grad64.abs().amax(-1).min()) > 0.0
    # The CPU fp32 product path factors the healthy rows too.
    _, _, info, _ = cpu_stages(case)
    assert info[[0, 2]].tolist() == [0, 0], case.name


def test_nan_row_fails_on_the_cpu_path_too():
  """The contract the GPU is held to, on the torch path: +inf and a zero
  gradient in the failed row, the others untouched."""
  case = fc.nan_case(97)
  base = fc.make_fit_case(97, *fc.NAN_GROUP)
  nll, grad = gp_model.nll_value_and_grad(case.raw, case.x, case.y)
  want_nll, want_grad = fc.cpu_fp32(base)
  assert float(nll[1]) == math.inf and bool((grad[1] == 0).all())
  assert torch.equal(nll[[0, 2]], want_nll[[0, 2]])
  assert torch.equal(grad[[0, 2]], want_grad[[0, 2]])


def test_gate_cases_have_an_oracle_away_from_zero():
  """The gate tests ask for 1e-3 relative of the oracle NLL."""
  for case in gate_cases():
    nll64 = fc.oracle_nll(case)
    assert bool(torch.isfinite(nll64).all())
    assert float(nll64.abs().min()) > 1.0, (case.name, nll64.tolist())


# -- the bounds see the slips they are there for --------------------------------


def test_solve_bound_sees_another_rows_mean():
  """z of restart r solved against restart 0's mean leaves the z bound in
  every case (the means differ by at least 1e-4:
  test_cases_are_what_they_claim)."""
  for case in fc.all_fit_cases():
    _, L, _, z = cpu_stages(case)
    p = gp_model.GPParams.from_raw(case.raw)
    for r in (1, 2):
      wrong = torch.linalg.solve_triangular(
          L[r], (case.y - p.mean[0]).unsqueeze(-1), upper=False).squeeze(-1)
      assert fc.solve_ratio(L[r], wrong, case.y, p.mean[r]) > 1.0, case.name


def test_nll_bound_sees_a_wrong_regulariser_and_another_rows_value():
  """Another restart's NLL leaves the bound in every case. 0.02 |raw|^2 for
  0.01 |raw|^2 leaves it wherever 0.01 |raw|^2 is above fp32 resolution of
  the NLL (at |nll| ~ 800 and |raw|^2 ~ 0.6 it is not): in most restarts."""
  seen = total = 0
  for case in fc.all_fit_cases():
    nll, L, _, z = cpu_stages(case)
    reg = (case.raw * case.raw).sum(-1)
    for r in range(3):
      assert fc.nll_ratio(nll[(r + 1) % 3], L[r], z[r],
                          case.raw[r]) > 1.0, case.name
      total += 1
      seen += fc.nll_ratio(nll[r] + 0.01 * reg[r], L[r], z[r],
                           case.raw[r]) > 1.0
  print(f'OBSERVED a doubled regulariser leaves the NLL bound in {seen} of '
        f'{total} restarts')
  assert seen >= 0.8 * total


def test_forward_criterion_sees_a_dropped_noise_term():
  """sum(M * K) without - noise tr(M) as the amplitude gradient: the error
  against the oracle is beyond 4x the CPU fp32 group worst in every group,
  so the GPU-only `k0 is None` branch cannot lose the term unseen."""
  for group in fc.GROUPS:
    gw, _ = fc.cpu_group_worst(*group)
    worst = 0.0
    for case in fc.group_cases(*group):
      _, grad64 = fc.oracle(case)
      raw, x, y = case.raw.double(), case.x.double(), case.y.double()
      p = gp_model.GPParams.from_raw(raw)
      K = gp_model.gram_matern52(x.unsqueeze(0), None, p.lengthscales,
                                 p.amplitude)
      K = K + p.noise.reshape(-1, 1, 1) * torch.eye(case.n, dtype=K.dtype)
      W = torch.linalg.inv(K)
      alpha = W @ (y.unsqueeze(0) - p.mean.unsqueeze(-1)).unsqueeze(-1)
      tr_m = (W - alpha @ alpha.mT).diagonal(dim1=-2, dim2=-1).sum(-1)
      sig = torch.sigmoid(raw[:, 0])
      chain = (gp_model._LOG_AMP_BOUNDS[1] - gp_model._LOG_AMP_BOUNDS[0]) * \
          sig * (1 - sig)
      wrong = grad64.clone()
      wrong[:, 0] += p.noise * tr_m * chain
      worst = max(worst, float(fc.grad_error(wrong, grad64).max()))
    print(f'OBSERVED {group}: dropped noise term {worst:.3e}, 4x the CPU '
          f'fp32 group worst {fc.MARGIN * gw:.3e}')
    assert worst > fc.MARGIN * gw, (group, worst, gw)
