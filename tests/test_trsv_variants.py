"""The two kernels behind ext.batched_trsv_lower give the same bits.

variant 0 (default) keeps every row's accumulator and its L columns in
registers and prefetches one panel ahead; variant 1 stages L through LDS
and keeps the right-hand side in global memory. Both compute, for row i,

  acc = b[i]; acc = fmaf(-L[i][j], z[j], acc) for j = 0 .. i-1; z[i] = acc /
  L[i][i]

in that order, so the results must be equal, not close.

Sizes: a partial and an exact 32-panel (1, 2, 31, 32, 33, 63, 64, 65), one
row into a second row per thread (255, 256, 257; 513 for a third), rows
whose length is no multiple of 4 (scalar loads) next to ones that are
(float4 loads), the production shape (1000), the last panel and the row
count at both sides of 1024, what gp_model dispatches at most (1200), and
both sides of the fall-back to variant 1 (1280, 1281).
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513, 1000, 1023, 1024,
         1200, 1280, 1281]


@pytest.fixture(scope='module')
def ext():
  from vizier_amd._src.ops import dispatch
  return dispatch.require_ext()  # Fails loudly if the .so is missing.


@functools.lru_cache(maxsize=None)
def factors(n):
  """(5, n, n) CPU fp32 Cholesky factors of A A^T / 48 + I, and (5, n) b."""
  g = torch.Generator().manual_seed(4000 + n)
  A = torch.randn(5, n, 48, generator=g)
  K = A @ A.mT / 48 + torch.eye(n)
  return torch.linalg.cholesky(K).contiguous(), torch.randn(5, n, generator=g)


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('R', [1, 5])
def test_variants_give_equal_bits(ext, R, n):
  L, b = factors(n)
  L, b = L[:R].cuda(), b[:R].cuda()
  z0 = ext.batched_trsv_lower(L, b, variant=0)
  z1 = ext.batched_trsv_lower(L, b, variant=1)
  assert bool(torch.isfinite(z1).all())
  assert torch.equal(z0, z1)
  # The default is variant 0.
  assert torch.equal(ext.batched_trsv_lower(L, b), z0)
  # The strict upper triangle, diagonal blocks included, is never used.
  poisoned = L.clone()
  upper = torch.ones(n, n, dtype=torch.bool, device='cuda').triu(1)
  poisoned[:, upper] = float('nan')
  assert torch.equal(ext.batched_trsv_lower(poisoned, b, variant=0), z1)
  assert torch.equal(ext.batched_trsv_lower(poisoned, b, variant=1), z1)


@pytest.mark.parametrize('n', [97, 321, 1000])
def test_variants_on_the_kernels_own_factor(ext, n):
  """On the L that batched_potrf returns, upper triangle as it left it."""
  g = torch.Generator().manual_seed(5000 + n)
  A = torch.randn(3, n, 48, generator=g)
  K = (A @ A.mT / 48 + torch.eye(n)).cuda()
  b = torch.randn(3, n, generator=g).cuda()
  L, info = ext.batched_potrf(K)
  assert info.tolist() == [0, 0, 0]
  z0 = ext.batched_trsv_lower(L, b, variant=0)
  z1 = ext.batched_trsv_lower(L, b, variant=1)
  assert bool(torch.isfinite(z1).all())
  assert torch.equal(z0, z1)
