"""batched_chol.hip (default v2 potrf, trsv) against float64 references.

Every reference is computed on the CPU in float64 from the float32 inputs.
With u = 2^-24 and gamma(k) = k u / (1 - k u), the bounds are Higham,
Accuracy and Stability of Numerical Algorithms (2nd ed.):

  potrf  |L L^T - K|_ij <= gamma(n + 1) (|L| |L|^T)_ij     (Thm 10.3)
  trsv   |b - L z|_i    <= gamma(n) (|L| |z|)_i            (Thm 8.5)

They hold for any summation order and with fma, so they need no
measurement. On top of the first, the kernel's worst ratio to that bound
may be at most 4x the ratio of the CPU fp32 LAPACK factor of the same
matrix: the two differ in blocking, summation order and fma contraction
only. `pytest -rA` prints both ratios per case as OBSERVED lines.

Matrices: Matern-5/2 grams of x ~ U[0, 1]^(n x d) built in float64 plus
noise * I, rounded to fp32 (cond 2e4 .. 1e6 at n = 321 .. 545, what the GP
fit factors), and the well-conditioned A A^T / k + I family of
test_gpu_ops.py. Only the lower triangle of the returned L is defined;
nothing here looks at the strict upper part.

The sizes cover a single partial panel (1, 2, 31), an exact panel (32), a
panel plus one row (33), the same one panel up (63, 64, 65, 96, 97: a last
panel of width 1), exactly one 256-row tile (288), a second tile of one
row (289), the last size with one row tile per round (320), the first with
two (321: also beyond the 64-column trailing tile), three row tiles (545),
and the production shapes (1000, 1024 = the cap).
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24

# (d, lengthscale, amplitude, noise)
MATERN = {
    'm52-d6-ls0.7': (6, 0.7, 1.3, 1e-3),
    'm52-d6-ls1.5': (6, 1.5, 1.3, 1e-5),
    'm52-d3-ls0.3': (3, 0.3, 0.8, 1e-2),
}
FAMILIES = list(MATERN) + ['aat']
SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 288, 289, 320, 321, 545,
         1000, 1024]
SMALL = [n for n in SIZES if n < 1000]
LARGE = [n for n in SIZES if n >= 1000]


def gamma(k):
  return k * U / (1.0 - k * U)


@pytest.fixture(scope='module')
def ext():
  from vizier_amd._src.ops import dispatch
  return dispatch.require_ext()  # Fails loudly if the .so is missing.


@functools.lru_cache(maxsize=None)
def matrix(family, n):
  """One (n, n) fp32 CPU matrix of the family (seeded by family and n)."""
  from vizier_amd._src.gp import matern
  g = torch.Generator().manual_seed(1000 * FAMILIES.index(family) + n)
  if family == 'aat':
    A = torch.randn(n, 48, generator=g)
    return (A @ A.mT / 48 + torch.eye(n)).contiguous()
  d, ls, amp, noise = MATERN[family]
  x = torch.rand(n, d, generator=g, dtype=torch.float64)
  K = matern.gram_matern52(
      x, None, torch.full((d,), ls, dtype=torch.float64),
      torch.tensor(amp, dtype=torch.float64))
  K = K + noise * torch.eye(n, dtype=torch.float64)
  return K.float().contiguous()


def backward_ratio(L, K):
  """max_ij |L L^T - K|_ij / (gamma(n + 1) (|L| |L|^T)_ij) over the lower
  triangle, in float64, from the lower triangle of L alone."""
  n = K.shape[-1]
  L64 = torch.tril(L.double())
  err = (L64 @ L64.mT - K.double()).abs()
  scale = gamma(n + 1) * (L64.abs() @ L64.abs().mT)
  return float(torch.tril(err / scale).max())


@functools.lru_cache(maxsize=None)
def lapack_ratio(family, n):
  """The same ratio for the CPU fp32 LAPACK factor; the precondition that
  fp32 can factor the matrix at all is asserted here."""
  K = matrix(family, n)
  L, info = torch.linalg.cholesky_ex(K)
  assert int(info) == 0, f'CPU fp32 potrf fails on {family} n={n}'
  return backward_ratio(L, K)


@functools.lru_cache(maxsize=None)
def reference_factor(family, n):
  """fp64 Cholesky factor of the fp32 matrix, rounded to fp32 (CPU)."""
  return torch.linalg.cholesky(matrix(family, n).double()).float()


def potrf(ext, K):
  L, info = ext.batched_potrf(K.cuda().contiguous())
  return L.cpu(), info.cpu()


def check_factor(tag, L, info, family, n):
  """info, diagonal, Higham's bound and the 4x-of-LAPACK bound."""
  K = matrix(family, n)
  assert int(info) == 0
  assert bool((L.diagonal() > 0).all())
  got, ref = backward_ratio(L, K), lapack_ratio(family, n)
  print(f'OBSERVED potrf {tag} {family} n={n}: kernel {got:.4f} of the '
        f'bound, CPU fp32 LAPACK {ref:.4f}')
  assert got <= 1.0, (family, n, got)
  assert got <= 4.0 * ref, (family, n, got, ref)


def lower_equal(a, b):
  """Bitwise equality of the lower triangles (the defined part)."""
  return torch.equal(torch.tril(a), torch.tril(b))


# -- batched_potrf ---------------------------------------------------------------


@pytest.mark.parametrize('n', SMALL)
def test_potrf_small(ext, n):
  """R = 1 per family against the bounds; R = 3 (distinct matrices) and
  R = 16 (every family four times) bitwise equal to the R = 1 factors."""
  alone = {}
  for family in FAMILIES:
    L, info = potrf(ext, matrix(family, n)[None])
    check_factor('R=1', L[0], info[0], family, n)
    alone[family] = L[0]
  three = list(MATERN)
  L, info = potrf(ext, torch.stack([matrix(f, n) for f in three]))
  assert info.tolist() == [0, 0, 0]
  for r, family in enumerate(three):
    assert lower_equal(L[r], alone[family]), (family, r)
  sixteen = FAMILIES * 4
  L, info = potrf(ext, torch.stack([matrix(f, n) for f in sixteen]))
  assert info.tolist() == [0] * 16
  for r, family in enumerate(sixteen):
    assert lower_equal(L[r], alone[family]), (family, r)
  # R copies of ONE matrix: workgroups of different matrices never mix.
  L, info = potrf(ext, matrix(three[1], n).expand(3, n, n))
  for r in range(3):
    assert lower_equal(L[r], alone[three[1]]), r


@pytest.mark.parametrize('n', LARGE)
def test_potrf_large(ext, n):
  """The production sizes, at R = 3 only: one matrix per Matern family,
  then three copies of one of them."""
  three = list(MATERN)
  L, info = potrf(ext, torch.stack([matrix(f, n) for f in three]))
  for r, family in enumerate(three):
    check_factor('R=3', L[r], info[r], family, n)
  copies, info = potrf(ext, matrix(three[0], n).expand(3, n, n))
  assert info.tolist() == [0, 0, 0]
  for r in range(3):
    assert lower_equal(copies[r], L[0]), r


INFO_CASES = [(64, 1), (64, 32), (64, 33), (64, 64), (97, 97), (321, 300),
              (321, 321)]


@pytest.mark.parametrize('n,col', INFO_CASES)
def test_potrf_info_is_the_first_failing_column(ext, n, col):
  """info is the 1-based first column whose pivot is not > 0: negative,
  zero and NaN all count, the smaller of two bad columns wins, and the
  other matrices of the batch are untouched by the failure."""
  family = 'm52-d6-ls0.7'
  good = matrix(family, n)
  clean, info = potrf(ext, torch.stack([good, matrix('aat', n)]))
  assert info.tolist() == [0, 0]

  negative = good.clone()
  negative[col - 1, col - 1] = -1.0
  # A zero pivot needs exact cancellation: the identity with one zero.
  zero = torch.eye(n)
  zero[col - 1, col - 1] = 0.0
  nan = good.clone()
  nan[col - 1, col - 1] = float('nan')
  bad = [negative, zero, nan]
  if col < n:
    two = negative.clone()
    two[n - 1, n - 1] = -1.0           # a later bad column does not win
    bad.append(two)
  for k, K in enumerate(bad):
    L, info = potrf(ext, torch.stack([good, K, matrix('aat', n)]))
    assert info.tolist() == [0, col, 0], (k, info.tolist())
    assert lower_equal(L[0], clean[0]) and lower_equal(L[2], clean[1]), k
    # Columns before the failing one do not depend on it.
    if k != 1 and col > 1:
      assert torch.equal(torch.tril(L[1])[:, :col - 1],
                         torch.tril(clean[0])[:, :col - 1]), k


def test_potrf_rejects_empty_batches(ext):
  with pytest.raises(RuntimeError, match='R >= 1 and N >= 1'):
    ext.batched_potrf(torch.empty(0, 8, 8, device='cuda'))
  with pytest.raises(RuntimeError, match='R >= 1 and N >= 1'):
    ext.batched_potrf(torch.empty(2, 0, 0, device='cuda'))
  with pytest.raises(RuntimeError, match='R >= 1 and N >= 1'):
    ext.batched_trsv_lower(torch.empty(0, 8, 8, device='cuda'),
                           torch.empty(0, 8, device='cuda'))
  with pytest.raises(RuntimeError, match='R >= 1 and N >= 1'):
    ext.batched_trsv_lower(torch.empty(2, 0, 0, device='cuda'),
                           torch.empty(2, 0, device='cuda'))


def test_potrf_more_workgroups_than_the_chip_holds(ext):
  """n = 321 runs round 0 on a (R, 2) grid; at R = 2048 that is 4096
  workgroups of ~38 KB LDS each (about 4 per CU, ~1000 resident: computed
  from the declared LDS arrays, not measured), blockIdx.x fastest. The
  y = 1 workgroups of the first matrices start after their y = 0 partners
  have finished, so a panel kernel that wrote the factored diagonal block
  in place would hand them an already factored block. The panel kernel
  did exactly that before it parked the block in a scratch tensor: on an
  MI355X this test then failed with info == 289 (the first column of the
  second row tile) for all 2048 copies of a matrix that factors alone."""
  family, n, R = 'm52-d6-ls0.7', 321, 2048
  K = matrix(family, n)
  alone, info = potrf(ext, K[None])
  check_factor('R=1', alone[0], info[0], family, n)
  big = K.cuda().expand(R, n, n).contiguous()
  L, info = ext.batched_potrf(big)
  del big
  assert int(info.abs().sum()) == 0
  want = alone[0].cuda()
  upper = torch.ones(n, n, dtype=torch.bool, device='cuda').triu(1)
  same = ((L == want) | upper).all(dim=2).all(dim=1)
  wrong = (~same).nonzero().flatten().tolist()
  del L
  torch.cuda.empty_cache()
  assert not wrong, f'{len(wrong)} of {R} factors differ, first {wrong[:8]}'


# -- batched_trsv_lower ------------------------------------------------------------


def trsv_residual_ratio(L, z, b):
  """max_i |b - L z|_i / (gamma(n) (|L| |z|)_i) from tril(L), float64."""
  n = L.shape[-1]
  L64 = torch.tril(L.double())
  z64, b64 = z.double(), b.double()
  res = (b64 - (L64 @ z64.unsqueeze(-1)).squeeze(-1)).abs()
  scale = gamma(n) * (L64.abs() @ z64.abs().unsqueeze(-1)).squeeze(-1)
  return float((res / scale).max())


@pytest.mark.parametrize('n', SIZES)
def test_trsv_lower(ext, n):
  g = torch.Generator().manual_seed(7000 + n)
  for R in (1, 5):
    families = [FAMILIES[(r + 1) % len(FAMILIES)] for r in range(R)]
    L = torch.stack([reference_factor(f, n) for f in families])
    b = torch.randn(R, n, generator=g)
    z = ext.batched_trsv_lower(L.cuda(), b.cuda()).cpu()
    ratio = trsv_residual_ratio(L, z, b)
    print(f'OBSERVED trsv R={R} n={n}: {ratio:.4f} of the bound')
    assert bool(torch.isfinite(z).all()) and ratio <= 1.0
    # The strict upper triangle is never read.
    poisoned = L.clone()
    poisoned[:, torch.ones(n, n, dtype=torch.bool).triu(1)] = float('nan')
    z_nan = ext.batched_trsv_lower(poisoned.cuda(), b.cuda()).cpu()
    assert torch.equal(z_nan, z)


@pytest.mark.parametrize('n', [33, 97, 321, 545, 1000])
def test_trsv_of_the_kernels_own_factor(ext, n):
  """z = trsv(potrf(K).L, b) with the upper triangle as potrf left it:
  the composition nll_values_with_chol runs."""
  three = list(MATERN)
  g = torch.Generator().manual_seed(9000 + n)
  K = torch.stack([matrix(f, n) for f in three]).cuda()
  b = torch.randn(3, n, generator=g)
  L, info = ext.batched_potrf(K)
  assert info.tolist() == [0, 0, 0]
  z = ext.batched_trsv_lower(L, b.cuda()).cpu()
  ratio = trsv_residual_ratio(L.cpu(), z, b)
  print(f'OBSERVED trsv(potrf) n={n}: {ratio:.4f} of the bound')
  assert bool(torch.isfinite(z).all()) and ratio <= 1.0
