"""Inputs, fp64 oracles and derived error bounds for the Matern-5/2 gram kernels.

Kernels: gram_matern52.hip (fp32 single and batched-restart), and the
bf16 / fp8 MFMA grams (gram_matern52_{bf16,fp8}{,_tiled}.hip). Shared by
tests/test_gram_cases.py (CPU) and tests/test_gram_kernels.py (GPU). Nothing
here touches the GPU.

Inputs
------
`make_case(n, m, d)`: x ~ U[0, 1]^d, lengthscales 0.6 sqrt(d) U(0.7, 1.4), so
that the scaled distance s = sqrt5 r is O(1) at every d (E d^2 = d / (6 ls^2)
~ 0.45) and most entries of K lie well inside (0, amp^2). Up to eight rows of
the longer operand are then replaced, as far as it has room (at most a quarter of
its rows, in the order far, dup, near; fewer than four rows: none):
  dup   an exact copy of a row of the other operand (d^2 = 0),
  near  that row + 2^-10 ls N(0, 1): d^2 ~ 1e-6 d, where n1 + n2 - 2 dot
        cancels almost completely,
  far   that row + ls v s / sqrt5, |v| = 1, s = 25 or 17: the planted pair
        has sqrt5 r in [15, 30]. The point leaves the unit box; the kernels
        do not care.
Cases of at least 64 entries are required (test_gram_cases.py) to have half
their entries in [0.05, 0.95] amp^2 and one below 1e-6 amp^2; smaller ones
cannot hold all three kinds of rows.

`make_exact_case(n, m, d, levels)`: x = k ls 2^-p with integer k in
[0, levels], ls a power of two per dimension, amp a power of two, p chosen
for s = O(1), plus duplicate rows. z = x / ls = k 2^-p is exact in bf16 for
levels = 32 and, after the scale max|z| / 8 = 2^-p, in e4m3 for levels = 8;
all differences, products, norms and dots are small integers times 4^-p and
exact in fp32. d^2 is therefore exact in every kernel, which can then differ
from fp64 only through its epilogue. No far rows here: they would leave the
integer range.

Oracles (fp64, from the fp32 inputs)
------------------------------------
fp32 kernels: vizier_amd/_src/gp/matern.py::gram_matern52 on `.double()`
inputs, + noise I and the gradient factor G = amp^2 (5/3)(1 + s) e^-s for
the batched kernel. MFMA kernels: `mfma_oracle` takes the ROUNDED operands
(bf16 or e4m3 bits as the binding builds them, and the fp8 scale) and
computes d^2 = scale^2 (|q1|^2 + |q2|^2 - 2 q1.q2) and the Matern function
in fp64. Rounding happens in `bf16_operands` / `fp8_operands`, the same
elementwise torch ops as the binding, on whatever device the inputs are on:
the GPU test rounds on the GPU and carries the bits over, so a 1-ulp
difference in a division cannot flip a rounding.

Bound (per entry)
-----------------
u = 2^-24, gamma(k) = k u / (1 - k u) (Higham, Accuracy and Stability of
Numerical Algorithms, Lemma 3.1). Write k(d^2) = (1 + s + s^2/3) e^-s,
s = sqrt(5 d^2). Then dk/d(d^2) = -(5/6)(1 + s) e^-s, for the gradient factor
g = (5/3)(1 + s) e^-s, dg/d(d^2) = -(25/6) e^-s; both magnitudes decrease
in d^2.

1. d^2. fp32 kernels sum squares of ((a - b) * fl(1 / ls)): three roundings
   per difference, doubled by the square, and a D-term fma sum with no
   cancellation: |d^2_hat - d^2| <= E = gamma(D + 8) d^2 (relative).
   MFMA kernels: the norms are fp32 sums over Dp exact products (fp8: of
   fl(q s)^2, three more roundings), the dot is an fp32 accumulation over
   Dp exact products in an order we do not know, and n1 + n2 - 2 scale2 dot
   adds four roundings: E = gamma(Dp + 8) (n1 + n2 + 2 |z1|.|z2|)
   (absolute; z = q scale, so scale^2 is included). Clamping at 0 only moves
   d^2_hat towards d^2 >= 0.
2. Through the function, by the mean value theorem with the derivative at
   its worst point of [d^2 - E, d^2 + E] clamped at 0, i.e. the lower end:
   P = amp^2 |dk/d(d^2)|(max(d^2 - E, 0)) E.
3. Epilogue: sqrt, the sqrt5 and 1/3 constants, the polynomial (about six
   roundings), fl(amp^2), the noise add, and the argument of the
   exponential, whose rounding error u s becomes a relative error u s of
   the result: C_EPI u (1 + s_hi) (|value| + P), C_EPI = 8,
   s_hi = sqrt(5 (d^2 + E)).
4. An absolute floor 2^-126 max(1, amp^2): below the smallest normal fp32
   number the relative statement stops.

bound = P + epilogue + floor. It is relative in nature: an entry of 1e-8
amp^2 is held to about 1e-8 of the tolerance of an entry near amp^2. For the
exact family E = 0 and only 3 and 4 remain.

What the derivation cannot fix is the accuracy of the fast exponential
(__expf) and of the MFMA's internal accumulation, which are not documented.
So on top of `<= 1.0 of the bound per case`, the GPU tests require the
kernel's worst ratio over a group of cases to be at most 4x the worst ratio
of `reference_fp32` / `mfma_reference_fp32` (the same formula in CPU fp32
torch, same operands) over the same group. Worst-of-group, not per case: in
a case of one or a few entries the CPU value is often correctly rounded by
chance and its ratio says nothing. The CPU reference itself must stay below
1.0 on every case (test_gram_cases.py).

Finding kept here because it explains the fp8 kernels' shape: with the fp8
MFMA (mfma_f32_16x16x32_fp8_fp8) the fp8 grams measured up to 4.8 of this
bound where the CPU reference has 0.35. Backing the dot out of the kernel's
output showed a one-sided error, up to 2^-12.4 of the largest product of a
K-step too low: the instruction sums its 32 products in a truncating
internal format (subnormal flushing was ruled out). The kernels now decode
e4m3 to bf16 in registers and use the bf16 MFMA, which meets step 1.
"""

import dataclasses
import functools
import math
from typing import Optional

import torch

U = 2.0 ** -24
SQRT5 = math.sqrt(5.0)
C_D2 = 8
C_EPI = 8
FLOOR = 2.0 ** -126
LS_C = 0.6
AMP = 1.3
FEATURES = ('far', 'dup', 'near', 'near', 'dup', 'far', 'near', 'dup')

# fp32 single-call kernel: 16 x 16 tiles, D staged in chunks of 32.
FP32_D = [1, 31, 32, 33, 64, 65]
FP32_SHAPES = [(1, 1), (1, 40), (40, 1), (15, 17), (16, 16), (17, 33),
               (64, 32), (128, 128),   # 8 and 64 workgroups: swizzled
               (65, 32), (48, 48)]     # 10 and 9: not
SYM_N = [1, 16, 17, 64, 100, 128]
SYM_D = [1, 33]
# Batched kernel: n = 64 is 16 workgroups per restart (swizzled), 100 is 49.
BATCHED_N = [1, 15, 16, 17, 64, 100]
BATCHED_D = [1, 32, 33, 65]
BATCHED_R = [1, 3]
# Strip MFMA kernels: 16 rows x (4 waves x 16 columns) per block. m = 1 .. 17
# leave waves 1 .. 3 without columns (early return), 63 and 65 clamp rows of
# the last wave, 130 is three blocks; (128, 64) is 8 workgroups: swizzled.
STRIP_N = [1, 15, 16, 17, 33]
STRIP_M = [1, 15, 16, 17, 63, 64, 65, 130]
STRIP_D = [1, 31, 32, 33, 65]
STRIP_SWIZZLED = (128, 64)
# Tiled MFMA kernels: 128 x 128 per block. (130, 400) is 8 workgroups
# (swizzled), (300, 260) is 9.
TILED_SHAPES = [(1, 1), (63, 65), (127, 129), (128, 128), (129, 127),
                (130, 400), (300, 260)]
TILED_D = [20, 33, 90]


def gamma(k):
  return k * U / (1.0 - k * U)


def padded(d):
  return (d + 31) // 32 * 32


def strip_shapes():
  return [(n, m) for n in STRIP_N for m in STRIP_M] + [STRIP_SWIZZLED]


@dataclasses.dataclass
class Case:
  name: str
  x1: torch.Tensor        # (n, d) fp32, CPU
  x2: torch.Tensor        # (m, d) fp32, CPU; the same object as x1 if sym
  ls: torch.Tensor        # (d,) fp32
  amp: float
  sym: bool = False
  exact: bool = False
  planted: tuple = ()     # (kind, row of x1, row of x2)

  @property
  def shape(self):
    return self.x1.shape[0], self.x2.shape[0], self.x1.shape[1]


def _seed(n, m, d, salt):
  return ((n * 1009 + m) * 1013 + d) * 7 + salt


def _plant_rows(g, target, source, ls, sym):
  """Overwrites rows of `target` from rows of `source`; returns the list of
  (kind, source row, target row)."""
  nt, ns, d = target.shape[0], source.shape[0], target.shape[1]
  count = min(len(FEATURES), nt // 4)
  if count == 0 or (sym and nt < 2):
    return []
  rows = torch.randperm(nt, generator=g)[:count].tolist()
  if nt - 1 not in rows:
    rows[-1] = nt - 1            # the last (edge) row is always one of them
  free = [i for i in range(ns) if not (sym and i in rows)]
  planted = []
  far_s = [25.0, 17.0]
  for kind, row in zip(FEATURES, rows):
    src = free[int(torch.randint(len(free), (1,), generator=g))]
    base = source[src].clone()
    if kind == 'near':
      base = base + 2.0 ** -10 * ls * torch.randn(d, generator=g)
    elif kind == 'far':
      v = torch.randn(d, generator=g)
      v = v / v.norm()
      base = base + ls * v * (far_s[len([p for p in planted
                                         if p[0] == 'far']) % 2] / SQRT5)
    target[row] = base
    planted.append((kind, src, row))
  return planted


@functools.lru_cache(maxsize=None)
def make_case(n, m, d, sym=False, salt=0):
  """The random family (module docstring). sym: x2 is x1 (m must equal n)."""
  g = torch.Generator().manual_seed(_seed(n, m, d, salt))
  ls = (LS_C * math.sqrt(d) *
        (0.7 + 0.7 * torch.rand(d, generator=g))).float()
  x1 = torch.rand(n, d, generator=g)
  if sym:
    assert n == m
    planted = [(k, s, t) for k, s, t in _plant_rows(g, x1, x1, ls, True)]
    x2 = x1
  else:
    x2 = torch.rand(m, d, generator=g)
    if m >= n:
      planted = _plant_rows(g, x2, x1, ls, False)
    else:
      planted = [(k, t, s) for k, s, t in _plant_rows(g, x1, x2, ls, False)]
  return Case(f'rand-{n}x{m}x{d}' + ('-sym' if sym else ''), x1, x2, ls, AMP,
              sym=sym, planted=tuple(planted))


@functools.lru_cache(maxsize=None)
def make_exact_case(n, m, d, levels=32, sym=False, salt=0):
  """The exact-operand family (module docstring). levels = 32 for the fp32
  and bf16 kernels, 8 for fp8 (max|z| / 8 is then the power of two 2^-p)."""
  assert levels in (8, 32)
  g = torch.Generator().manual_seed(_seed(n, m, d, salt + 3))
  ls = 2.0 ** torch.randint(-1, 2, (d,), generator=g).float()
  p = round(0.5 * math.log2(d * levels * (levels + 2) / 2.7))
  k1 = torch.randint(0, levels + 1, (n, d), generator=g).float()
  k1[0, 0] = levels                      # max|z| = levels 2^-p exactly
  if sym:
    assert n == m
    k2 = k1
    pairs = [(i, n - 1 - i) for i in range(1, min(3, n // 2))]
    for i, j in pairs:
      k1[j] = k1[i]
  else:
    k2 = torch.randint(0, levels + 1, (m, d), generator=g).float()
    pairs = [(i % n, m - 1 - i) for i in range(min(3, m, n))]
    for i, j in pairs:
      k2[j] = k1[i]
  x1 = k1 * ls * 2.0 ** -p
  x2 = x1 if sym else k2 * ls * 2.0 ** -p
  amp = 2.0 if (n + m + d) % 2 == 0 else 0.5
  return Case(f'exact{levels}-{n}x{m}x{d}' + ('-sym' if sym else ''), x1, x2,
              ls, amp, sym=sym, exact=True,
              planted=tuple(('dup', i, j) for i, j in pairs))


def batched_params(case, r):
  """Distinct (ls (r, d), amp (r,), noise (r,)) fp32 per restart for the
  batched kernel over case.x1. Powers of two for the exact family."""
  if case.exact:
    f = torch.tensor([1.0, 2.0, 0.5])[:r]
    amp = torch.tensor([2.0, 0.5, 1.0])[:r]
  else:
    f = torch.tensor([1.0, 0.6, 1.7])[:r]
    amp = torch.tensor([1.3, 0.4, 2.5])[:r]
  noise = torch.tensor([1e-3, 0.25, 1e-6])[:r]
  return (f[:, None] * case.ls[None, :]).contiguous(), amp, noise


# -- the Matern function and its derivative magnitudes, any float dtype ------


def k_of_d2(d2):
  s = (5.0 * d2).sqrt()
  return (1.0 + s + s * s / 3.0) * torch.exp(-s)


def g_of_d2(d2):
  s = (5.0 * d2).sqrt()
  return (5.0 / 3.0) * (1.0 + s) * torch.exp(-s)


def _dk(d2):
  s = (5.0 * d2).sqrt()
  return (5.0 / 6.0) * (1.0 + s) * torch.exp(-s)


def _dg(d2):
  return (25.0 / 6.0) * torch.exp(-(5.0 * d2).sqrt())


def value_bound(d2, err_d2, amp2, value, deriv=_dk):
  """Steps 2-4 of the module docstring. d2, err_d2, value: fp64 (..., n, m);
  amp2 broadcastable; value = the oracle entries (noise included)."""
  amp2 = torch.as_tensor(amp2, dtype=torch.float64)
  prop = amp2 * deriv((d2 - err_d2).clamp_min(0.0)) * err_d2
  s_hi = (5.0 * (d2 + err_d2)).sqrt()
  epilogue = C_EPI * U * (1.0 + s_hi) * (value.abs() + prop)
  return prop + epilogue + FLOOR * amp2.clamp_min(1.0)


def worst_ratio(got, want, bound):
  """max |got - want| / bound over all entries, in fp64. NaN or inf in got
  gives inf."""
  got = got.double()
  if not bool(torch.isfinite(got).all()):
    return math.inf
  if got.numel() == 0:
    return 0.0
  return float(((got - want).abs() / bound).max())


# -- fp32 kernels ------------------------------------------------------------


def diff_d2(x1, x2, ls):
  """fp64 squared scaled distances in the difference form, (..., n, m)."""
  z1 = x1.double() / ls.double().unsqueeze(-2)
  z2 = x2.double() / ls.double().unsqueeze(-2)
  diff = z1.unsqueeze(-2) - z2.unsqueeze(-3)
  return (diff * diff).sum(-1)


def oracle_fp32(case):
  """fp64 K (n, m) of the single-call kernel."""
  from vizier_amd._src.gp import matern
  return matern.gram_matern52(
      case.x1.double(), None if case.sym else case.x2.double(),
      case.ls.double(), torch.tensor(case.amp, dtype=torch.float64))


def bound_fp32(case):
  d2 = diff_d2(case.x1, case.x2, case.ls)
  err = torch.zeros_like(d2) if case.exact else \
      gamma(case.shape[2] + C_D2) * d2
  return value_bound(d2, err, case.amp ** 2, oracle_fp32(case))


def _epilogue_fp32(d2, amp2):
  """The kernels' epilogue in fp32 torch: (poly, exp) of sr."""
  sr = torch.tensor(SQRT5, dtype=torch.float32) * d2.clamp_min(0.0).sqrt()
  third = torch.tensor(1.0, dtype=torch.float32) / 3.0
  e = torch.exp(-sr)
  return amp2 * ((1.0 + sr + sr * sr * third) * e), sr, e


def _diff_d2_fp32(x1, x2, ls):
  inv = 1.0 / ls.float().unsqueeze(-2)
  diff = (x1.float().unsqueeze(-2) - x2.float().unsqueeze(-3)) * \
      inv.unsqueeze(-2)
  return (diff * diff).sum(-1)


def reference_fp32(case):
  """The single-call kernel's formula in CPU fp32 torch."""
  amp2 = torch.tensor(case.amp * case.amp, dtype=torch.float32)
  return _epilogue_fp32(_diff_d2_fp32(case.x1, case.x2, case.ls), amp2)[0]


def oracle_batched(case, ls, amp, noise):
  """fp64 (K (r, n, n) with noise on the diagonal, G (r, n, n))."""
  from vizier_amd._src.gp import matern
  x = case.x1.double()
  n = x.shape[0]
  K = matern.gram_matern52(x.unsqueeze(0), None, ls.double(), amp.double())
  K = K + noise.double().reshape(-1, 1, 1) * torch.eye(
      n, dtype=torch.float64)
  d2 = diff_d2(x.unsqueeze(0), x.unsqueeze(0), ls)
  G = (amp.double() ** 2).reshape(-1, 1, 1) * g_of_d2(d2)
  return K, G


def bound_batched(case, ls, amp, noise):
  x = case.x1.unsqueeze(0)
  d2 = diff_d2(x, x, ls)
  err = torch.zeros_like(d2) if case.exact else \
      gamma(case.shape[2] + C_D2) * d2
  amp2 = (amp.double() ** 2).reshape(-1, 1, 1)
  K, G = oracle_batched(case, ls, amp, noise)
  return (value_bound(d2, err, amp2, K),
          value_bound(d2, err, amp2, G, deriv=_dg))


def reference_batched(case, ls, amp, noise):
  """The batched kernel's formula in CPU fp32 torch: (K, G)."""
  x = case.x1.unsqueeze(0)
  amp2 = (amp.float() * amp.float()).reshape(-1, 1, 1)
  K, sr, e = _epilogue_fp32(_diff_d2_fp32(x, x, ls), amp2)
  K = K + noise.float().reshape(-1, 1, 1) * torch.eye(case.shape[0])
  G = amp2 * (torch.tensor(5.0, dtype=torch.float32) / 3.0) * \
      (1.0 + sr) * e
  return K, G


# -- MFMA kernels ------------------------------------------------------------


def _pad_cast(z, dtype):
  n, d = z.shape
  out = torch.zeros(n, padded(d), dtype=dtype, device=z.device)
  out[:, :d] = z.to(dtype)
  return out


def bf16_operands(x1, x2, ls):
  """(z1b, z2b): (x / ls).to(bfloat16), zero-padded to Dp, as the binding
  builds them; on the device of the inputs."""
  return (_pad_cast(x1 / ls, torch.bfloat16),
          _pad_cast(x2 / ls, torch.bfloat16))


def fp8_operands(x1, x2, ls):
  """(z1q, z2q, scale) as gram_matern52_fp8 builds them: scale =
  max(max|z| / 8, 1e-8) as a double, q = (z / scale).to(float8_e4m3fn)."""
  z1, z2 = x1 / ls, x2 / ls
  s = max(float(z1.abs().max()), float(z2.abs().max())) / 8.0
  s = max(s, 1e-8)
  return (_pad_cast(z1 / s, torch.float8_e4m3fn),
          _pad_cast(z2 / s, torch.float8_e4m3fn), s)


def cache_scale(ls):
  """Fp8GramCache's fixed unit-box scale."""
  return max(float((1.0 / ls).max()) / 8.0, 1e-8)


def fp8_operand(x, ls, scale):
  """One operand quantised at a given scale, as Fp8GramCache does."""
  return _pad_cast((x / ls) / scale, torch.float8_e4m3fn)


def fp32_norms(q, scale=1.0):
  """The binding's fp32 row norms of the rounded operand."""
  zf = q.to(torch.float32) * scale
  return (zf * zf).sum(-1)


@dataclasses.dataclass
class MfmaRef:
  d2: torch.Tensor       # (n, m) fp64, clamped at 0
  k: torch.Tensor        # (n, m) fp64 oracle
  bound: torch.Tensor    # (n, m) fp64


def mfma_oracle(q1, q2, amp, scale=1.0, exact=False,
                n1: Optional[torch.Tensor] = None,
                n2: Optional[torch.Tensor] = None):
  """fp64 oracle and bound from the rounded operands q1 (n, Dp), q2 (m, Dp)
  (bf16 or e4m3, CPU) and the fp8 scale. n1 / n2 override the norms (fp64)
  to build the deliberately wrong oracle of test_gram_cases.py."""
  z1 = q1.cpu().to(torch.float32).double() * scale
  z2 = q2.cpu().to(torch.float32).double() * scale
  m1 = (z1 * z1).sum(-1) if n1 is None else n1.double()
  m2 = (z2 * z2).sum(-1) if n2 is None else n2.double()
  d2 = (m1[:, None] + m2[None, :] - 2.0 * (z1 @ z2.mT)).clamp_min(0.0)
  k = amp ** 2 * k_of_d2(d2)
  if exact:
    err = torch.zeros_like(d2)
  else:
    err = gamma(q1.shape[1] + C_D2) * (
        m1[:, None] + m2[None, :] + 2.0 * (z1.abs() @ z2.abs().mT))
  return MfmaRef(d2, k, value_bound(d2, err, amp ** 2, k))


def mfma_reference_fp32(q1, q2, amp, scale=1.0):
  """n1 + n2 - 2 z1f @ z2f.T and the epilogue in CPU fp32 torch, from the
  same rounded operands."""
  z1 = q1.cpu().to(torch.float32) * scale
  z2 = q2.cpu().to(torch.float32) * scale
  n1, n2 = (z1 * z1).sum(-1), (z2 * z2).sum(-1)
  d2 = n1[:, None] + n2[None, :] - 2.0 * (z1 @ z2.mT)
  amp2 = torch.tensor(amp * amp, dtype=torch.float32)
  return _epilogue_fp32(d2, amp2)[0]
