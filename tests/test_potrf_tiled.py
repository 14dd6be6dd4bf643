"""batched_potrf v6 (tiled trailing update, column-wise panel solve) against v2.

v6 runs v2's rounds with another work split and operand schedule and, element
by element, v2's floating-point operations in v2's order, so the lower
triangle of L and info are BIT-equal; nothing here has a tolerance. Both run
in one process through the binding's `impl` argument. How good the factor is
(Higham's bounds, the info semantics, batch independence, 4096 workgroups) is
held by test_chol_kernels.py on the default path, which is v6.

Matrices: the families of test_chol_kernels.py, built by its `matrix`
(same seeding), and their images under reversing the point order
(P K P^T: the gram of the same points listed backwards), which makes the
batches of distinct matrices. Each matrix is asserted to factor in CPU fp32
LAPACK with info == 0.

Sizes: a single partial panel (1, 31); the exact panel and a one-row panel
tile (32, 33); a trailing matrix of 32 and 33 rows (64, 65); of 63 and 64
rows, then a second 64-tile of one row and a last panel of width 1 (95, 96,
97); three tile pairs with a partial last tile (128, 129); 160, 161; the
row-tile boundaries of a panel kernel with 256 rows per workgroup (v2) and,
with 97 and 161, of one with 64 (v6) (289, 321); 545; the production shape
and the cap (1000, 1024). n % 4 == 0 takes the float4 paths, the others the
scalar ones.
"""

import functools

import pytest
import torch

import test_chol_kernels as ck

pytestmark = pytest.mark.gpu

WORST, AAT = 'm52-d6-ls1.5', 'aat'
OTHERS = [f for f in ck.FAMILIES if f not in (WORST, AAT)]
SMALL = [1, 31, 32, 33, 64, 65, 95, 96, 97, 128, 129, 160, 161, 289, 321,
         545]
ALL_FAMILIES_AT = (97, 161, 321)
LARGE = [(1000, 8), (1024, 2)]
V6 = ['v6']


@pytest.fixture(scope='module')
def ext():
  from vizier_amd._src.ops import dispatch
  return dispatch.require_ext()  # Fails loudly if the .so is missing.


@functools.lru_cache(maxsize=None)
def matrix(family, n, flipped=False):
  """ck.matrix(family, n), or that with the point order reversed; the
  precondition that CPU fp32 LAPACK factors it is asserted here."""
  K = ck.matrix(family, n)
  if flipped:
    K = K.flip(0, 1).contiguous()
  assert int(torch.linalg.cholesky_ex(K).info) == 0, (family, n, flipped)
  return K


def batch(family, n, R):
  """R matrices, the first three distinct (for n > 1): the family's, its
  reversed image and the reversed image of another family."""
  other = AAT if family != AAT else WORST
  three = [matrix(family, n), matrix(family, n, True), matrix(other, n, True)]
  return torch.stack([three[r % 3] for r in range(R)])


def potrf(ext, K, impl):
  L, info = ext.batched_potrf(K.cuda().contiguous(), impl)
  return torch.tril(L).cpu(), info.cpu()


def assert_same_bits(ext, K, tag):
  want, want_info = potrf(ext, K, 'v2')
  assert want_info.tolist() == [0] * K.shape[0], tag
  for impl in V6:
    got, info = potrf(ext, K, impl)
    assert torch.equal(info, want_info), (tag, impl, info.tolist())
    for r in range(K.shape[0]):
      if not torch.equal(got[r], want[r]):
        bad = (got[r] != want[r]).nonzero()
        raise AssertionError(
            f'{tag} {impl}: matrix {r} differs from v2 at {len(bad)} '
            f'elements, first (row, column) {bad[0].tolist()}')


@pytest.mark.parametrize('n', SMALL)
def test_v6_is_bitwise_v2(ext, n):
  families = [WORST, AAT] + (OTHERS if n in ALL_FAMILIES_AT else [])
  for family in families:
    for R in (1, 3, 9):
      assert_same_bits(ext, batch(family, n, R), f'{family} n={n} R={R}')


@pytest.mark.parametrize('n,R', LARGE)
def test_v6_is_bitwise_v2_at_the_production_sizes(ext, n, R):
  for family in (WORST, AAT):
    assert_same_bits(ext, batch(family, n, R), f'{family} n={n} R={R}')


def test_default_is_v6(ext):
  K = batch(WORST, 161, 3)
  L, info = ext.batched_potrf(K.cuda())
  want, want_info = potrf(ext, K, 'v6')
  assert torch.equal(torch.tril(L).cpu(), want)
  assert torch.equal(info.cpu(), want_info)
  for retired in ('v3', 'v4', 'v5', 'v7'):
    with pytest.raises(RuntimeError, match='impl must be one of'):
      ext.batched_potrf(K.cuda(), retired)


@pytest.mark.parametrize('pivot', [-1.0, float('nan')])
def test_a_failing_pivot_is_reported_alike(ext, pivot):
  """n = 161, pivot 100 of matrix 1 of 3 is bad: info [0, 100, 0] from v2
  and v6, the neighbours untouched, and the columns before the bad one
  equal bit for bit."""
  n, col = 161, 100
  good, last = matrix(WORST, n), matrix(AAT, n)
  bad = good.clone()
  bad[col - 1, col - 1] = pivot
  if pivot < 0:
    assert int(torch.linalg.cholesky_ex(bad).info) == col
  clean = {impl: potrf(ext, torch.stack([good, last]), impl)[0]
           for impl in ['v2'] + V6}
  K = torch.stack([good, bad, last])
  want, want_info = potrf(ext, K, 'v2')
  assert want_info.tolist() == [0, col, 0]
  for impl in V6:
    got, info = potrf(ext, K, impl)
    assert info.tolist() == [0, col, 0], (impl, info.tolist())
    assert torch.equal(got[0], clean[impl][0]), impl
    assert torch.equal(got[2], clean[impl][1]), impl
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    assert torch.equal(got[1][:, :col - 1], want[1][:, :col - 1]), impl


def ceil_div(a, b):
  return -(-a // b)


def test_launch_shape(ext):
  """What the launcher runs in round 0 (the largest round), from the
  binding's host-side query: 64 x 64 tile pairs of the trailing matrix's
  lower triangle, panel row tiles, and the scratch for parked diagonal
  blocks exactly when a round has more than one panel row tile."""
  default = ext.batched_potrf_launch_shape(1000)
  assert default == ext.batched_potrf_launch_shape(1000, 'v6')
  assert default == [64, 16, 136, 1]  # 16 tiles of 64 cover 968 rows
  assert ext.batched_potrf_launch_shape(1000, 'v2') == [256, 4, 16, 1]
  sizes = sorted(set(SMALL + [n for n, _ in LARGE] +
                     [2, 63, 288, 320, 2000] + list(range(90, 100)) +
                     list(range(286, 292))))
  for impl, rows in [('v6', 64), ('v2', 256)]:
    for n in sizes:
      got_rows, row_tiles, trailing, scratch = (
          ext.batched_potrf_launch_shape(n, impl))
      below = max(n - 32, 0)            # rows under round 0's block
      assert got_rows == rows
      assert row_tiles == max(ceil_div(below, rows), 1), (impl, n)
      t = ceil_div(below, 64)
      assert trailing == (t if impl == 'v2' else t * (t + 1) // 2), (impl, n)
      assert scratch == int(row_tiles > 1), (impl, n)
