"""The line-search ladder hands z = L^-1 (y - mean) over with its factor.

`nll_value_and_grad(chol_hint=(L, info))` solves L z = resid itself;
`chol_hint=(L, info, z)` may take the ladder's z, which solved the same
system on the same L at the same raw values. Unlike a hint against no hint
(where the two build K differently,
test_gp_core.test_chol_hint_matches_no_hint), the results must be equal,
not close.

z is taken over only where both sides run the HIP solve (fp32, GPU, more
than one restart): one kernel, one L, one resid. torch's solve_triangular
rounds differently for the ladder's cholesky_ex output and for the
gathered copy the hint path holds, so on that path (every CPU case here)
the three-member hint solves again, and equality then says that the third
member is accepted and changes nothing.
"""

import pytest
import torch

from vizier_amd._src.gp import gp_model
from vizier_amd._src.gp import lbfgs


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
@pytest.mark.parametrize('restarts', [1, 3])
def test_three_member_hint_equals_two_member_hint(dtype, restarts):
  g = torch.Generator().manual_seed(5)
  x = torch.rand(40, 3, generator=g).to(dtype)
  y = torch.randn(40, generator=g).to(dtype)
  raw = (torch.randn(restarts, 6, generator=g) * 0.5).to(dtype)
  nll_l, L, info, z = gp_model.nll_values_with_chol_z(raw, x, y)
  # The three-value form the existing callers use is unchanged.
  nll_3, L_3, info_3 = gp_model.nll_values_with_chol(raw, x, y)
  assert torch.equal(nll_3, nll_l) and torch.equal(L_3, L)
  assert torch.equal(info_3, info)
  nll_2, grad_2 = gp_model.nll_value_and_grad(
      raw, x, y, chol_hint=(L, info))
  nll_z, grad_z = gp_model.nll_value_and_grad(
      raw, x, y, chol_hint=(L, info, z))
  assert bool(torch.isfinite(nll_2).all())
  assert torch.equal(nll_z, nll_2)
  assert torch.equal(grad_z, grad_2)


@pytest.mark.gpu
@pytest.mark.parametrize('n', [97, 1000])
def test_three_member_hint_equals_two_member_hint_on_the_hip_solve(n):
  """fp32 on the GPU with more than one restart runs batched_potrf and
  batched_trsv_lower, and only there is z taken over instead of solved
  again (on torch's solve the two would differ in the last bits)."""
  g = torch.Generator().manual_seed(11)
  x = torch.rand(n, 4, generator=g).cuda()
  y = torch.randn(n, generator=g).cuda()
  raw = (torch.randn(3, 7, generator=g) * 0.5).cuda()
  _, L, info, z = gp_model.nll_values_with_chol_z(raw, x, y)
  assert z.shape == (3, n)  # The HIP solve's layout.
  nll_2, grad_2 = gp_model.nll_value_and_grad(
      raw, x, y, chol_hint=(L, info))
  nll_z, grad_z = gp_model.nll_value_and_grad(
      raw, x, y, chol_hint=(L, info, z))
  assert bool(torch.isfinite(nll_2).all())
  assert torch.equal(nll_z, nll_2)
  assert torch.equal(grad_z, grad_2)


def test_ladder_rows_selected_with_their_z():
  """lbfgs picks the accepted row of every cache member alike, z
  included: a ladder that returns (L, info, z) reaches the same optimum
  as one that returns (L, info)."""
  g = torch.Generator().manual_seed(7)
  x = torch.rand(30, 2, generator=g).double()
  y = torch.sin(4 * x[:, 0]).double()
  raw0 = torch.randn(2, 5, generator=g).double() * 0.4

  def loss_fn(raw):
    return gp_model.negative_log_marginal_likelihood(raw, x, y)

  def vag(raw, hint=None):
    return gp_model.nll_value_and_grad(raw, x, y, chol_hint=hint)

  def ladder2(raw):
    nll_v, L, info = gp_model.nll_values_with_chol(raw, x, y)
    return nll_v, (L, info)

  def ladder3(raw):
    nll_v, L, info, z = gp_model.nll_values_with_chol_z(raw, x, y)
    return nll_v, (L, info, z)

  best_2, f_2 = lbfgs.minimize_batched(
      loss_fn, raw0.clone(), max_iters=15, value_and_grad_fn=vag,
      ladder_fn=ladder2)
  best_3, f_3 = lbfgs.minimize_batched(
      loss_fn, raw0.clone(), max_iters=15, value_and_grad_fn=vag,
      ladder_fn=ladder3)
  assert torch.equal(f_3, f_2)
  assert torch.equal(best_3, best_2)
