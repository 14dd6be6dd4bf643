"""The Matern-5/2 gram kernels against quantisation-exact fp64 oracles.

gram_matern52.hip (fp32 single call and batched restarts) and the bf16 / fp8
MFMA grams, strip and LDS-tiled, through every binding: gram_matern52,
gram_matern52_batched, gram_matern52_bf16{,_tiled}, gram_matern52_fp8{,_tiled},
gram_matern52_fp8_pre and acquisitions.Fp8GramCache.

Inputs, oracles and the derived per-entry bound are in tests/gram_cases.py
(derivation in its docstring; its CPU conditions in tests/test_gram_cases.py).
Every comparison uses ALL entries. The bf16 / fp8 operands are rounded here
with torch on the GPU, by the same elementwise ops as the bindings, and the
bits go to the fp64 oracle: what is left between kernel and oracle is fp32
accumulation and the epilogue.

Per case the kernel must stay within 1.0 of the bound. Per test (a group of
cases of one kernel) its worst ratio may be at most 4x the worst ratio of the
CPU fp32 torch evaluation of the same formula on the same operands.
`pytest -rA` prints both per case as OBSERVED lines.

Shapes are the smallest that reach each branch; the lists and what each
member is for are in gram_cases.py.
"""

import math

import pytest
import torch

import gram_cases as gc

pytestmark = pytest.mark.gpu

EXACT_SHAPES = [(17, 33), (33, 65), (128, 64)]
EXACT_TILED_SHAPES = [(63, 65), (129, 127)]


@pytest.fixture(scope='module')
def ext():
  from vizier_amd._src.ops import dispatch
  return dispatch.require_ext()  # Fails loudly if the .so is missing.


def poison(*shape):
  """Fills a block of the output's size with NaN and frees it. The caching
  allocator usually hands it to the binding's torch.empty, so an entry the
  kernel fails to write tends to be NaN and not a correct leftover of the
  previous call at the same shape."""
  torch.full(shape, float('nan'), device='cuda')


class Group:
  """Worst ratios of one kernel over the cases of one test."""

  def __init__(self, kernel):
    self.kernel, self.got, self.ref = kernel, 0.0, 0.0

  def check(self, name, got, want, bound, cpu_ref):
    got = got.cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    r = gc.worst_ratio(got, want, bound)
    c = gc.worst_ratio(cpu_ref, want, bound)
    print(f'OBSERVED {self.kernel} {name}: kernel {r:.4f} of the bound, '
          f'CPU fp32 {c:.4f}')
    assert r <= 1.0, (self.kernel, name, r)
    self.got, self.ref = max(self.got, r), max(self.ref, c)

  def finish(self):
    print(f'OBSERVED {self.kernel} worst of the group: kernel '
          f'{self.got:.4f}, CPU fp32 {self.ref:.4f}')
    assert self.got <= 4.0 * self.ref, (self.kernel, self.got, self.ref)


def on_gpu(case):
  x1 = case.x1.cuda()
  x2 = x1 if case.sym else case.x2.cuda()
  return x1, x2, case.ls.cuda()


# -- fp32 gram_matern52 --------------------------------------------------------------


def run_fp32(ext, group, case):
  x1, x2, ls = on_gpu(case)
  n, m, _ = case.shape
  poison(n, m)
  got = ext.gram_matern52(x1, x2, ls, case.amp)
  group.check(case.name, got, gc.oracle_fp32(case), gc.bound_fp32(case),
              gc.reference_fp32(case))
  return got


@pytest.mark.parametrize('d', gc.FP32_D)
def test_fp32_gram(ext, d):
  group = Group('gram_matern52')
  for n, m in gc.FP32_SHAPES:
    run_fp32(ext, group, gc.make_case(n, m, d))
  group.finish()


@pytest.mark.parametrize('d', gc.FP32_D)
def test_fp32_gram_exact_operands(ext, d):
  """d^2 is exact: the kernel differs from fp64 through its epilogue alone,
  and coincident rows give exactly amp^2."""
  group = Group('gram_matern52 exact')
  for n, m in EXACT_SHAPES:
    case = gc.make_exact_case(n, m, d, 32)
    got = run_fp32(ext, group, case).cpu()
    for _, i, j in case.planted:
      assert float(got[i, j]) == case.amp ** 2
  group.finish()


@pytest.mark.parametrize('n', gc.SYM_N)
def test_fp32_symmetric_path(ext, n):
  """x1 and x2 the same tensor: only the upper tiles are computed and
  mirrored. Bitwise symmetric, bitwise the non-symmetric call on a copy
  (both square the same difference in the same order), bitwise what
  dispatch.gram_matern52(x, None) returns, and inside the bound."""
  from vizier_amd._src.ops import dispatch
  group = Group('gram_matern52 sym')
  for d in gc.SYM_D:
    case = gc.make_case(n, n, d, sym=True)
    x, _, ls = on_gpu(case)
    K = run_fp32(ext, group, case)
    assert torch.equal(K, K.T), case.name
    poison(n, n)
    assert torch.equal(K, ext.gram_matern52(x, x.clone(), ls, case.amp)), \
        case.name
    poison(n, n)
    assert torch.equal(
        K, dispatch.gram_matern52(
            x, None, ls, torch.tensor(case.amp, dtype=torch.float64))), \
        case.name
    assert torch.equal(K.diagonal().cpu(), torch.full(
        (n,), case.amp * case.amp, dtype=torch.float32)), case.name
  group.finish()


# -- gram_matern52_batched -------------------------------------------------------------


@pytest.mark.parametrize('exact', [False, True], ids=['random', 'exact'])
@pytest.mark.parametrize('d', gc.BATCHED_D)
def test_batched_gram(ext, d, exact):
  """R = 1 and 3 restarts with distinct lengthscales, amplitudes and noises,
  with and without the gradient factor. K and G against the bound, bitwise
  symmetric; K the same bits whether or not G is asked for; the noise on
  the diagonal only (off the diagonal K has the bits of a call with zero
  noise)."""
  gk, gg = Group('batched K'), Group('batched G')
  for n in gc.BATCHED_N:
    case = gc.make_exact_case(n, n, d, 32, sym=True) if exact else \
        gc.make_case(n, n, d, sym=True)
    x = case.x1.cuda()
    for r in gc.BATCHED_R:
      ls, amp, noise = gc.batched_params(case, r)
      want_k, want_g = gc.oracle_batched(case, ls, amp, noise)
      bound_k, bound_g = gc.bound_batched(case, ls, amp, noise)
      ref_k, ref_g = gc.reference_batched(case, ls, amp, noise)
      args = (x, ls.cuda(), amp.cuda())
      poison(r, n, n)
      (K_only,) = ext.gram_matern52_batched(*args, noise.cuda(), False)
      poison(r, n, n)
      poison(r, n, n)
      K, G = ext.gram_matern52_batched(*args, noise.cuda(), True)
      name = f'{case.name} R={r}'
      gk.check(name, K, want_k, bound_k, ref_k)
      gg.check(name, G, want_g, bound_g, ref_g)
      assert torch.equal(K, K_only), name
      assert torch.equal(K, K.mT) and torch.equal(G, G.mT), name
      (K0,) = ext.gram_matern52_batched(*args, torch.zeros(r).cuda(), False)
      off = ~torch.eye(n, dtype=torch.bool, device='cuda')
      assert torch.equal(K[:, off], K0[:, off]), name
      if exact:   # coincident rows: exactly amp^2 (+ noise on the diagonal)
        amp2 = (amp * amp).cuda()
        for _, i, j in case.planted:
          assert torch.equal(K[:, i, j], amp2), name
        assert torch.equal(K0.diagonal(dim1=1, dim2=2),
                           amp2[:, None].expand(r, n)), name
  gk.finish()
  gg.finish()


def test_batched_restart_matches_single_call(ext):
  """Restart r of the batched kernel and the single-call kernel at the same
  parameters take different epilogue code (inline vs matern52_of_d2), so
  they are not compared bit for bit: each is held to the bound."""
  group = Group('batched vs single')
  case = gc.make_case(100, 100, 33, sym=True)
  ls, amp, noise = gc.batched_params(case, 3)
  (K,) = ext.gram_matern52_batched(case.x1.cuda(), ls.cuda(), amp.cuda(),
                                   torch.zeros(3).cuda(), False)
  for r in range(3):
    one = gc.Case(f'{case.name} r={r}', case.x1, case.x1, ls[r],
                  float(amp[r]), sym=True)
    want, bound = gc.oracle_fp32(one), gc.bound_fp32(one)
    ref = gc.reference_fp32(one)
    group.check(one.name + ' batched', K[r], want, bound, ref)
    run_fp32(ext, group, one)
  group.finish()


# -- bf16 / fp8 MFMA grams ---------------------------------------------------------------


def mfma_call(ext, kind, entry, case, group, exact=False):
  """One call of a bf16 / fp8 binding against the oracle built from the
  operands rounded on the GPU. entry: '' (dispatcher: strip below 512 rows),
  '_tiled' or '_pre'."""
  x1, x2, ls = on_gpu(case)
  n, m, _ = case.shape
  if kind == 'bf16':
    q1, q2 = gc.bf16_operands(x1, x2, ls)
    s = 1.0
  else:
    q1, q2, s = gc.fp8_operands(x1, x2, ls)
  poison(n, m)
  if entry == '_pre':
    got = ext.gram_matern52_fp8_pre(q1, q2, gc.fp32_norms(q1, s),
                                    gc.fp32_norms(q2, s), case.amp, s)
  else:
    got = getattr(ext, f'gram_matern52_{kind}{entry}')(x1, x2, ls, case.amp)
  ref = gc.mfma_oracle(q1, q2, case.amp, s, exact=exact)
  group.check(case.name, got, ref.k, ref.bound,
              gc.mfma_reference_fp32(q1, q2, case.amp, s))
  return got, ref


MFMA_STRIP = [('bf16', ''), ('fp8', ''), ('fp8', '_pre')]
MFMA_TILED = [('bf16', '_tiled'), ('fp8', '_tiled'), ('fp8', '_pre')]


@pytest.mark.parametrize('kind,entry', MFMA_STRIP)
@pytest.mark.parametrize('d', gc.STRIP_D)
def test_mfma_strip(ext, kind, entry, d):
  """The strip kernels over n x m x D: a single row, partial and full
  16-row tiles, waves with no columns (early return), clamped rows and
  columns, one to three blocks across, Dp = 32, 64 and 96, and the 8
  workgroup grid that takes the swizzle."""
  group = Group(f'{kind}{entry} strip')
  for n, m in gc.strip_shapes():
    mfma_call(ext, kind, entry, gc.make_case(n, m, d), group)
  group.finish()


@pytest.mark.parametrize('kind,entry', MFMA_TILED)
@pytest.mark.parametrize('d', gc.TILED_D)
def test_mfma_tiled(ext, kind, entry, d):
  """The LDS-tiled kernels (and, for fp8_pre, the strip kernel at the same
  larger shapes): one partial tile, tiles one row or column short of, at and
  past 128, the swizzled 8 workgroup grid and the 9 workgroup one."""
  group = Group(f'{kind}{entry} tiled-shapes')
  for n, m in gc.TILED_SHAPES:
    mfma_call(ext, kind, entry, gc.make_case(n, m, d), group)
  group.finish()


@pytest.mark.parametrize('kind,entry,levels', [
    ('bf16', '', 32), ('bf16', '_tiled', 32), ('fp8', '', 8),
    ('fp8', '_tiled', 8), ('fp8', '_pre', 8)])
def test_mfma_exact_operands(ext, kind, entry, levels):
  """Rounding is a no-op and d^2 is exact in fp32: only the epilogue is
  left, and coincident rows give exactly amp^2 (d^2 is clamped from an exact
  0)."""
  group = Group(f'{kind}{entry} exact')
  for d in (33, 65):
    for n, m in EXACT_SHAPES + EXACT_TILED_SHAPES:
      case = gc.make_exact_case(n, m, d, levels)
      got, _ = mfma_call(ext, kind, entry, case, group, exact=True)
      for _, i, j in case.planted:
        assert float(got[i, j]) == case.amp ** 2, (case.name, i, j)
  group.finish()


@pytest.mark.parametrize('kind', ['bf16', 'fp8'])
def test_mfma_result_is_not_its_transpose(ext, kind):
  """A square cross-gram of two different operands: the transposed oracle
  must violate the bound, so a kernel that swapped rows and columns could
  not pass."""
  group = Group(f'{kind} strip')
  got, ref = mfma_call(ext, kind, '', gc.make_case(17, 17, 33), group)
  assert gc.worst_ratio(got.cpu(), ref.k.T, ref.bound.T) > 1.0


@pytest.mark.parametrize('kind', ['bf16', 'fp8'])
@pytest.mark.parametrize('n,m,d', [(63, 65, 33), (129, 127, 90),
                                   (130, 400, 20)])
def test_strip_and_tiled_are_bit_equal(ext, kind, n, m, d):
  """Both kernels run the same MFMA over k in the same order on the same
  operands and share the epilogue."""
  case = gc.make_case(n, m, d)
  x1, x2, ls = on_gpu(case)
  poison(n, m)
  strip = getattr(ext, f'gram_matern52_{kind}')(x1, x2, ls, case.amp)
  poison(n, m)
  tiled = getattr(ext, f'gram_matern52_{kind}_tiled')(x1, x2, ls, case.amp)
  diff = float((strip.double() - tiled.double()).abs().max())
  print(f'OBSERVED {kind} strip vs tiled {case.name}: max |diff| {diff:.3e}')
  assert torch.equal(strip, tiled), (case.name, diff)


@pytest.mark.parametrize('kind', ['bf16', 'fp8'])
def test_dispatcher_threshold(ext, kind):
  """gram_matern52_{bf16,fp8} take the tiled kernel from (512, 512) on and
  the strip kernel below. At (512, 512) the result has the bits of the
  explicit tiled entry point. At (511, 512) it has the bits of the strip
  kernel run on the two column halves (m = 256 < 512 is always strip, and an
  entry depends on its own row and column alone). Both meet the bound."""
  group = Group(f'{kind} dispatcher')
  case = gc.make_case(512, 512, 20)
  x1, x2, ls = on_gpu(case)
  got, _ = mfma_call(ext, kind, '', case, group)
  poison(512, 512)
  tiled = getattr(ext, f'gram_matern52_{kind}_tiled')(x1, x2, ls, case.amp)
  assert torch.equal(got, tiled)
  below = gc.Case('rand-511x512x20', case.x1[:511].contiguous(), case.x2,
                  case.ls, case.amp)
  got, _ = mfma_call(ext, kind, '', below, group)
  f = getattr(ext, f'gram_matern52_{kind}')
  x1b = x1[:511].contiguous()
  if kind == 'bf16':
    halves = [f(x1b, x2[:256].contiguous(), ls, case.amp),
              f(x1b, x2[256:].contiguous(), ls, case.amp)]
  else:               # per-call scales differ: use the pre-quantised entry
    q1, q2, s = gc.fp8_operands(x1b, x2, ls)
    n1, n2 = gc.fp32_norms(q1, s), gc.fp32_norms(q2, s)
    halves = [ext.gram_matern52_fp8_pre(q1, q2[:256].contiguous(), n1,
                                        n2[:256].contiguous(), case.amp, s),
              ext.gram_matern52_fp8_pre(q1, q2[256:].contiguous(), n1,
                                        n2[256:].contiguous(), case.amp, s)]
  assert torch.equal(got, torch.cat(halves, 1))
  group.finish()


def test_fp8_pre_takes_the_tiled_kernel_at_512(ext):
  group = Group('fp8_pre tiled')
  case = gc.make_case(512, 512, 33)
  got, _ = mfma_call(ext, 'fp8', '_pre', case, group)
  x1, x2, ls = on_gpu(case)
  assert torch.equal(got, ext.gram_matern52_fp8_tiled(x1, x2, ls, case.amp))
  group.finish()


@pytest.mark.parametrize('n,m,d', [(1, 1, 1), (17, 33, 33), (33, 130, 65),
                                   (130, 400, 90), (512, 512, 20)])
def test_fp8_gram_cache(ext, n, m, d):
  """Fp8GramCache.gram against the oracle built from cache.z2q, cache.scale
  and the candidate bits quantised here at that scale; cache.n2 against the
  fp64 norms of cache.z2q."""
  from vizier_amd._src.gp import acquisitions
  group = Group('Fp8GramCache')
  case = gc.make_case(n, m, d)
  x1, x2, ls = on_gpu(case)
  cache = acquisitions.Fp8GramCache(x2, ls, case.amp)
  assert cache.scale == gc.cache_scale(ls)
  assert cache.z2q.shape == (m, gc.padded(d))
  assert torch.equal(cache.z2q.view(torch.uint8),
                     gc.fp8_operand(x2, ls, cache.scale).view(torch.uint8))
  n2 = (cache.z2q.cpu().float().double() * cache.scale).pow(2).sum(-1)
  assert bool(((cache.n2.cpu().double() - n2).abs() <=
               gc.gamma(gc.padded(d) + 3) * n2).all())
  q1 = gc.fp8_operand(x1, ls, cache.scale)
  poison(n, m)
  got = cache.gram(x1)
  ref = gc.mfma_oracle(q1, cache.z2q, case.amp, cache.scale)
  group.check(case.name, got, ref.k, ref.bound,
              gc.mfma_reference_fp32(q1, cache.z2q, case.amp, cache.scale))
  group.finish()


@pytest.mark.parametrize('entry', ['', '_tiled'])
def test_fp8_all_zero_inputs(ext, entry):
  """max|z| = 0: the scale takes its floor 1e-8, every d^2 is 0 and every
  entry exactly amp^2."""
  x1, x2 = torch.zeros(17, 33).cuda(), torch.zeros(130, 33).cuda()
  ls = torch.full((33,), 0.7).cuda()
  poison(17, 130)
  got = getattr(ext, f'gram_matern52_fp8{entry}')(x1, x2, ls, 1.5)
  assert torch.equal(got.cpu(), torch.full((17, 130), 2.25))


# -- binding behaviour -----------------------------------------------------------------------


GRAMS = ['gram_matern52', 'gram_matern52_bf16', 'gram_matern52_bf16_tiled',
         'gram_matern52_fp8', 'gram_matern52_fp8_tiled']


@pytest.mark.parametrize('kind,entry', [('bf16', ''), ('bf16', '_tiled'),
                                        ('fp8', ''), ('fp8', '_tiled')])
def test_one_row_view_of_the_other_operand(ext, kind, entry):
  """x[:1] and x share a data pointer. The (1, m) cross-gram must be row 0
  of the square one (and meet the bound), not amp^2 everywhere: sharing a
  pointer makes x2 the same operand as x1 only if the shapes agree too."""
  case = gc.make_case(40, 40, 33, sym=True)
  x, _, ls = on_gpu(case)
  f = getattr(ext, f'gram_matern52_{kind}{entry}')
  assert x[:1].data_ptr() == x.data_ptr() and x[:1].is_contiguous()
  poison(1, 40)
  got = f(x[:1], x, ls, case.amp)
  assert got.shape == (1, 40)
  if kind == 'bf16':
    q1, q2 = gc.bf16_operands(x[:1], x, ls)
    s = 1.0
  else:
    q1, q2, s = gc.fp8_operands(x[:1], x, ls)
  ref = gc.mfma_oracle(q1, q2, case.amp, s)
  ratio = gc.worst_ratio(got.cpu(), ref.k, ref.bound)
  print(f'OBSERVED {kind}{entry} one-row view: kernel {ratio:.4f} of the '
        'bound')
  assert ratio <= 1.0
  assert torch.equal(got, f(x, x, ls, case.amp)[:1])


def test_fp32_one_row_view_of_the_other_operand(ext):
  """The fp32 binding takes its symmetric path only for equal row counts."""
  group = Group('gram_matern52 one-row view')
  case = gc.make_case(40, 40, 33, sym=True)
  x, _, ls = on_gpu(case)
  got = ext.gram_matern52(x[:1], x, ls, case.amp)
  one = gc.Case('rand-1x40x33-view', case.x1[:1], case.x1, case.ls, case.amp)
  group.check(one.name, got, gc.oracle_fp32(one), gc.bound_fp32(one),
              gc.reference_fp32(one))


@pytest.mark.parametrize('name', GRAMS)
def test_gram_bindings_reject_bad_operands(ext, name):
  """Each raises before anything is launched or indexed."""
  f = getattr(ext, name)
  x1, x2 = torch.rand(5, 4).cuda(), torch.rand(6, 4).cuda()
  ls = torch.ones(4).cuda()
  assert f(x1, x2, ls, 1.0).shape == (5, 6)
  with pytest.raises(RuntimeError, match='columns'):
    f(x1, torch.rand(6, 1).cuda(), ls, 1.0)      # would broadcast
  with pytest.raises(RuntimeError, match='columns'):
    f(x1, torch.rand(6, 5).cuda(), ls, 1.0)
  with pytest.raises(RuntimeError, match='lengthscales must have'):
    f(x1, x2, torch.ones(1).cuda(), 1.0)
  with pytest.raises(RuntimeError, match='2-D'):
    f(x1[0], x2, ls, 1.0)
  with pytest.raises(RuntimeError, match='2-D'):
    f(x1, x2[None], ls, 1.0)
  with pytest.raises(RuntimeError, match='2-D'):
    f(x1[None], x2[None], ls, 1.0)
  with pytest.raises(RuntimeError, match='GPU tensor'):
    f(x1.cpu(), x2, ls, 1.0)
  with pytest.raises(RuntimeError, match='GPU tensor'):
    f(x1, x2.cpu(), ls, 1.0)
  with pytest.raises(RuntimeError, match='GPU tensor'):
    f(x1, x2, ls.cpu(), 1.0)
  with pytest.raises(RuntimeError, match='fp32'):
    f(x1.double(), x2.double(), ls.double(), 1.0)


def test_dispatch_forwards_the_shape_check(ext):
  from vizier_amd._src.ops import dispatch
  x = torch.rand(2, 5, 4).cuda()
  with pytest.raises(RuntimeError, match='2-D'):
    dispatch.gram_matern52(x, None, torch.ones(4).cuda(), torch.tensor(1.0))


def test_batched_binding_rejects_bad_operands(ext):
  x = torch.rand(5, 4).cuda()
  ls, amp, noise = (torch.ones(2, 4).cuda(), torch.ones(2).cuda(),
                    torch.zeros(2).cuda())
  assert ext.gram_matern52_batched(x, ls, amp, noise, False)[0].shape == \
      (2, 5, 5)
  with pytest.raises(RuntimeError, match='2-D'):
    ext.gram_matern52_batched(x[0], ls, amp, noise, False)
  with pytest.raises(RuntimeError, match=r'\(R, D\)'):
    ext.gram_matern52_batched(x, ls[0], amp, noise, False)
  with pytest.raises(RuntimeError, match=r'\(R, D\)'):
    ext.gram_matern52_batched(x, torch.ones(2, 3).cuda(), amp, noise, False)
  with pytest.raises(RuntimeError, match=r'\(R, D\)'):
    ext.gram_matern52_batched(x, torch.ones(()).cuda(), amp, noise, False)
  with pytest.raises(RuntimeError, match=r'\(R,\)'):
    ext.gram_matern52_batched(x, ls, amp[:1], noise, False)
  with pytest.raises(RuntimeError, match=r'\(R,\)'):
    ext.gram_matern52_batched(x, ls, amp, torch.zeros(3).cuda(), False)
  with pytest.raises(RuntimeError, match='GPU tensor'):
    ext.gram_matern52_batched(x.cpu(), ls, amp, noise, False)


def test_fp8_pre_rejects_bad_operands(ext):
  case = gc.make_case(5, 6, 4)
  x1, x2, ls = on_gpu(case)
  q1, q2, s = gc.fp8_operands(x1, x2, ls)
  n1, n2 = gc.fp32_norms(q1, s), gc.fp32_norms(q2, s)
  f = ext.gram_matern52_fp8_pre
  assert f(q1, q2, n1, n2, 1.0, s).shape == (5, 6)
  with pytest.raises(RuntimeError, match='GPU tensors'):
    f(q1.cpu(), q2, n1, n2, 1.0, s)
  with pytest.raises(RuntimeError, match='GPU tensors'):
    f(q1, q2.cpu(), n1, n2, 1.0, s)
  with pytest.raises(RuntimeError, match='GPU tensor'):
    f(q1, q2, n1.cpu(), n2, 1.0, s)
  with pytest.raises(RuntimeError, match='GPU tensor'):
    f(q1, q2, n1, n2.cpu(), 1.0, s)
  with pytest.raises(RuntimeError, match='n1 must have 5'):
    f(q1, q2, n1[:4], n2, 1.0, s)
  with pytest.raises(RuntimeError, match='n1 must have 5'):
    f(q1, q2, n2, n2, 1.0, s)
  with pytest.raises(RuntimeError, match='n2 must have 6'):
    f(q1, q2, n1, n2[:1], 1.0, s)
  with pytest.raises(RuntimeError, match='multiple of 32'):
    f(q1[:, :16].contiguous(), q2[:, :16].contiguous(), n1, n2, 1.0, s)
  with pytest.raises(RuntimeError, match='multiple of 32'):
    f(q1, torch.cat([q2.view(torch.uint8)] * 2, 1).view(torch.float8_e4m3fn),
      n1, n2, 1.0, s)
  with pytest.raises(RuntimeError, match='2-D'):
    f(q1[0], q2, n1, n2, 1.0, s)
  with pytest.raises(RuntimeError, match='float8_e4m3fn'):
    f(q1.float(), q2, n1, n2, 1.0, s)


@pytest.mark.parametrize('n,m', [(0, 7), (7, 0), (0, 0)])
def test_empty_operands_give_empty_grams(ext, n, m):
  """No launch with an empty grid: an empty (n, m) result."""
  x1, x2 = torch.rand(n, 4).cuda(), torch.rand(m, 4).cuda()
  ls = torch.ones(4).cuda()
  for name in GRAMS:
    got = getattr(ext, name)(x1, x2, ls, 1.0)
    assert got.shape == (n, m) and got.dtype == torch.float32, name
    assert got.is_cuda
  q1 = torch.zeros(n, 32, dtype=torch.float8_e4m3fn, device='cuda')
  q2 = torch.zeros(m, 32, dtype=torch.float8_e4m3fn, device='cuda')
  got = ext.gram_matern52_fp8_pre(q1, q2, torch.zeros(n).cuda(),
                                  torch.zeros(m).cuda(), 1.0, 1.0)
  assert got.shape == (n, m)
  torch.cuda.synchronize()


def test_empty_batched_gram(ext):
  x = torch.rand(0, 4).cuda()
  ls, amp, noise = (torch.ones(2, 4).cuda(), torch.ones(2).cuda(),
                    torch.zeros(2).cuda())
  K, G = ext.gram_matern52_batched(x, ls, amp, noise, True)
  assert K.shape == (2, 0, 0) and G.shape == (2, 0, 0)
  (K,) = ext.gram_matern52_batched(torch.rand(5, 4).cuda(), ls[:0], amp[:0],
                                   noise[:0], False)
  assert K.shape == (0, 5, 5)
  torch.cuda.synchronize()


def test_fp32_gram_rejects_an_output_past_int_range(ext):
  """The kernel indexes out[row * m + col] in int: 46341^2 > 2^31 - 1 must
  raise, before the 8.6 GB output is allocated."""
  x = torch.rand(46341, 1).cuda()
  assert 46341 ** 2 >= 2 ** 31 > 46340 ** 2
  with pytest.raises(RuntimeError, match=r'2\^31'):
    ext.gram_matern52(x, x, torch.ones(1).cuda(), 1.0)
  assert math.isfinite(float(x.sum()))
