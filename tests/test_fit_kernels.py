"""The GPU GP fit (NLL, analytic gradient, ladder hints, gates) against fp64.

gp_model.nll_values_with_chol_z and gp_model.nll_value_and_grad chain
gram_matern52_batched, batched_potrf and batched_trsv_lower into the fit's
loss and gradient; the `k0 is None` amplitude-gradient branch of the latter
runs on the GPU fp32 path alone. Inputs, the fp64 autograd oracle and the
derivation of every bound are in tests/fit_cases.py (its CPU conditions in
tests/test_fit_cases.py). `pytest -rA` prints every figure as an OBSERVED
line.

A  Stage by stage (default mode, 30 cases of 3 restarts): K at the GPU's own
   fp32 parameters against gram_cases.bound_batched; L against Higham's
   backward bound and 4x the CPU fp32 LAPACK factor on the same K; z against
   the residual bound with ITS restart's mean; the returned NLL against its
   fp64 recomputation from the returned L, z and raw.
B  Forward accuracy of four routes (no hint, hint (L, info), hint (L, info,
   z), negative_log_marginal_likelihood) against the oracle: the worst over
   a (d, noise_rel) group may be at most 4x the worst of the CPU fp32
   product path over that group. Repeated for VIZIER_AMD_CUSTOM_CHOL=trsv
   and =0 on the d = 4 groups.
C  Bitwise equalities that follow from the code: hint against no hint, the
   ladder's NLL against the gradient evaluation's, VIZIER_AMD_TRSV=v1
   against the default, L-BFGS with and without the ladder.
D  A failed factorisation (NaN amplitude; duplicate rows at the noise floor)
   gives +inf and a zero gradient in its row and leaves the other rows inside
   A and B.
E  The gates: which of the three kernels ran, through a recording proxy of
   the extension, for every environment setting, size threshold, dtype and
   requires_grad.

Observed on the MI355X (kernel / CPU fp32 product path on the same machine;
the CPU figures move by up to 2x with the host's BLAS and thread count).
Forward, default mode, worst of the three gradient routes, which agree:

  group           gradient              NLL
  d1  noise 1e-1  3.2e-6 / 2.4e-6      2.1e-5 / 2.1e-5
  d1  noise 1e-3  8.1e-4 / 6.0e-4      8.3e-4 / 6.4e-4
  d4  noise 1e-1  4.5e-6 / 3.9e-6      6.2e-6 / 1.3e-5
  d4  noise 1e-3  4.3e-4 / 3.9e-4      2.6e-3 / 3.0e-3
  d33 noise 1e-1  2.2e-6 / 4.2e-6      2.3e-6 / 1.2e-6
  d33 noise 1e-3  4.6e-5 / 2.7e-5      7.1e-6 / 6.6e-6
  d4  1e-1 =trsv and =0   4.2e-6 / 3.9e-6      9.0e-6 / 1.3e-5
  d4  1e-3 =trsv and =0   8.7e-4 / 3.9e-4      3.1e-3 / 3.0e-3
  dup (noise 1e-2)        1.2e-4 / 1.0e-4      3.2e-5 / 4.9e-5

Stages, worst of 90 restarts, of the bound: K 0.51, L 0.49 (CPU fp32 LAPACK
0.58; at most 1.85x LAPACK's on the same K), z 0.34, NLL 0.11. The NaN row
reports info = 1; the near-singular row failed at all four sizes (info = n -
7 or n - 6: the first or second row that repeats an earlier one). Every
equality of part C held. Gates: every NLL within 1.8e-4 relative of the
oracle.
"""

import math

import pytest
import torch

import fit_cases as fc
import gram_cases as gc
from vizier_amd._src.gp import gp_model
from vizier_amd._src.gp import lbfgs

pytestmark = pytest.mark.gpu

GROUP_IDS = {g: f'd{g[0]}-noise{g[1]:g}' for g in fc.GROUPS}
ROUTES = ('no hint', 'hint (L, info)', 'hint (L, info, z)', 'nlml')
EQUAL_N = [97, 321]


@pytest.fixture(scope='module')
def ext():
  from vizier_amd._src.ops import dispatch
  return dispatch.require_ext()  # Fails loudly if the .so is missing.


def set_mode(monkeypatch, mode, trsv=None):
  """mode None: the default (variable unset)."""
  monkeypatch.delenv('VIZIER_AMD_CUSTOM_CHOL', raising=False)
  monkeypatch.delenv('VIZIER_AMD_TRSV', raising=False)
  if mode is not None:
    monkeypatch.setenv('VIZIER_AMD_CUSTOM_CHOL', mode)
  if trsv is not None:
    monkeypatch.setenv('VIZIER_AMD_TRSV', trsv)


def on_gpu(case):
  return case.raw.cuda(), case.x.cuda(), case.y.cuda()


class Run:
  """One case through the ladder call and the four routes in one mode;
  everything carried to the CPU."""

  def __init__(self, ext, case):
    raw, x, y = on_gpu(case)
    nll, L, info, z = gp_model.nll_values_with_chol_z(raw, x, y)
    self.z_shape = tuple(z.shape)
    p = gp_model.GPParams.from_raw(raw)
    (K,) = ext.gram_matern52_batched(
        x, p.lengthscales.contiguous(), p.amplitude.contiguous(),
        p.noise.contiguous(), False)
    self.ls, self.amp, self.noise, self.mean = (
        t.cpu() for t in (p.lengthscales, p.amplitude, p.noise, p.mean))
    self.K, self.nll, self.L, self.info = K.cpu(), nll.cpu(), L.cpu(), \
        info.cpu()
    self.z = z.reshape(z.shape[0], -1).cpu()
    self.routes = {
        'no hint': gp_model.nll_value_and_grad(raw, x, y),
        'hint (L, info)': gp_model.nll_value_and_grad(
            raw, x, y, chol_hint=(L, info)),
        'hint (L, info, z)': gp_model.nll_value_and_grad(
            raw, x, y, chol_hint=(L, info, z)),
        'nlml': (gp_model.negative_log_marginal_likelihood(raw, x, y), None),
    }
    self.routes = {k: (v[0].cpu(), None if v[1] is None else v[1].cpu())
                   for k, v in self.routes.items()}

  def healthy(self, case, route):
    rows = list(case.healthy)
    nll, grad = self.routes[route]
    return nll[rows], None if grad is None else grad[rows]


_RUNS = {}


def run_of(ext, monkeypatch, case, mode=None):
  """Each case runs once per mode; the result is shared and left unchanged."""
  set_mode(monkeypatch, mode)
  key = (case.name, mode)
  if key not in _RUNS:
    _RUNS[key] = Run(ext, case)
  return _RUNS[key]


def check_factor_solve_nll(case, run):
  """A.2 to A.4 on the healthy restarts of one default-mode run."""
  assert run.z_shape == (case.raw.shape[0], case.n)  # the HIP solve's layout
  for r in case.healthy:
    K, L, z = run.K[r], run.L[r], run.z[r]
    assert int(run.info[r]) == 0, (case.name, r, run.info.tolist())
    got, ref = fc.backward_ratio(L, K), fc.lapack_ratio(K)
    zr = fc.solve_ratio(L, z, case.y, run.mean[r])
    nr = fc.nll_ratio(run.nll[r], L, z, case.raw[r])
    print(f'OBSERVED stages {case.name} r={r}: L {got:.4f} of the bound '
          f'(CPU fp32 LAPACK {ref:.4f}), z {zr:.4f}, NLL {nr:.4f}')
    assert got <= 1.0, (case.name, r, got)
    assert got <= fc.MARGIN * ref, (case.name, r, got, ref)
    assert zr <= 1.0, (case.name, r, zr)
    assert nr <= 1.0, (case.name, r, nr)


def route_worsts(cases, runs):
  """{route: (worst gradient error, worst NLL error)} over the healthy
  restarts of the cases; no gradient for the value-only route."""
  out = {}
  for route in ROUTES:
    gw = nw = 0.0
    for case, run in zip(cases, runs):
      nll64, grad64 = fc.oracle(case)
      nll, grad = run.healthy(case, route)
      nw = max(nw, float(fc.nll_error(nll, nll64).max()))
      if grad is not None:
        gw = max(gw, float(fc.grad_error(grad, grad64).max()))
    out[route] = (gw if route != 'nlml' else None, nw)
  return out


def check_group(tag, worsts, cpu):
  """Prints every route's worst next to the CPU's, then asserts 4x."""
  for route, (gw, nw) in worsts.items():
    grad = '' if gw is None else f'grad {gw:.3e} (CPU fp32 {cpu[0]:.3e}), '
    print(f'OBSERVED forward {tag} {route}: {grad}nll {nw:.3e} (CPU fp32 '
          f'{cpu[1]:.3e})')
  for route, (gw, nw) in worsts.items():
    if gw is not None:
      assert gw <= fc.MARGIN * cpu[0], (tag, route, 'grad', gw, cpu[0])
    assert nw <= fc.MARGIN * cpu[1], (tag, route, 'nll', nw, cpu[1])


# -- A: stage by stage ---------------------------------------------------------------


@pytest.mark.parametrize('case', fc.all_fit_cases(), ids=lambda c: c.name)
def test_stages(ext, monkeypatch, case):
  run = run_of(ext, monkeypatch, case)
  # The parameters are the GPU's own bits: a 1-ulp sigmoid / exp difference
  # is not charged to a kernel (and is at most a few ulp of the CPU's).
  p = gp_model.GPParams.from_raw(case.raw)
  for got, want in ((run.ls, p.lengthscales), (run.amp, p.amplitude),
                    (run.noise, p.noise)):
    assert torch.allclose(got, want, rtol=1e-5, atol=0.0), case.name
  as_gram = gc.Case(case.name, case.x, case.x, run.ls[0], 1.0, sym=True)
  params = (run.ls, run.amp, run.noise)
  want_k, _ = gc.oracle_batched(as_gram, *params)
  bound_k, _ = gc.bound_batched(as_gram, *params)
  kr = gc.worst_ratio(run.K, want_k, bound_k)
  print(f'OBSERVED stages {case.name}: K {kr:.4f} of the bound')
  assert kr <= 1.0, (case.name, kr)
  check_factor_solve_nll(case, run)


# -- B: forward accuracy ---------------------------------------------------------------


@pytest.mark.parametrize('group', fc.GROUPS, ids=list(GROUP_IDS.values()))
def test_forward_accuracy(ext, monkeypatch, group):
  cases = fc.group_cases(*group)
  runs = [run_of(ext, monkeypatch, c) for c in cases]
  check_group(GROUP_IDS[group], route_worsts(cases, runs),
              fc.cpu_group_worst(*group))


@pytest.mark.parametrize('mode', ['trsv', '0'])
@pytest.mark.parametrize('group', [g for g in fc.GROUPS if g[0] == 4],
                         ids=lambda g: GROUP_IDS[g])
def test_forward_accuracy_other_modes(ext, monkeypatch, group, mode):
  """=trsv: the MAGMA factor and the HIP solve. =0: torch throughout (n =
  289 and 321 through the identity-padded factorisation)."""
  cases = fc.group_cases(*group)
  runs = [run_of(ext, monkeypatch, c, mode) for c in cases]
  for case, run in zip(cases, runs):
    want = (3, case.n) if mode == 'trsv' else (3, case.n, 1)
    assert run.z_shape == want, (case.name, run.z_shape)
    assert run.info.tolist() == [0, 0, 0], case.name
  check_group(f'{GROUP_IDS[group]} mode={mode}', route_worsts(cases, runs),
              fc.cpu_group_worst(*group))


# -- C: equalities ----------------------------------------------------------------------


def equal_case(n):
  return fc.make_fit_case(n, 4, 1e-3)


@pytest.mark.parametrize('n', EQUAL_N)
def test_ladder_hint_equals_no_hint(ext, monkeypatch, n):
  """Both sides build K with the same kernel (K has the same bits with and
  without G) and factor and solve it with the same kernels; the ladder's NLL
  is the gradient evaluation's."""
  set_mode(monkeypatch, None)
  raw, x, y = on_gpu(equal_case(n))
  nll_l, L, info, z = gp_model.nll_values_with_chol_z(raw, x, y)
  nll_0, grad_0 = gp_model.nll_value_and_grad(raw, x, y)
  nll_2, grad_2 = gp_model.nll_value_and_grad(raw, x, y, chol_hint=(L, info))
  nll_3, grad_3 = gp_model.nll_value_and_grad(
      raw, x, y, chol_hint=(L, info, z))
  assert info.tolist() == [0, 0, 0]
  assert bool(torch.isfinite(nll_0).all() and torch.isfinite(grad_0).all())
  assert torch.equal(nll_3, nll_0) and torch.equal(grad_3, grad_0)
  assert torch.equal(nll_2, nll_0) and torch.equal(grad_2, grad_0)
  assert torch.equal(nll_l, nll_0)


@pytest.mark.parametrize('n', EQUAL_N)
def test_trsv_v1_equals_default(ext, monkeypatch, n):
  raw, x, y = on_gpu(equal_case(n))
  set_mode(monkeypatch, None)
  nll_0, grad_0 = gp_model.nll_value_and_grad(raw, x, y)
  lad_0 = gp_model.nll_values_with_chol_z(raw, x, y)
  set_mode(monkeypatch, None, trsv='v1')
  nll_1, grad_1 = gp_model.nll_value_and_grad(raw, x, y)
  lad_1 = gp_model.nll_values_with_chol_z(raw, x, y)
  assert bool(torch.isfinite(nll_0).all())
  assert torch.equal(nll_1, nll_0) and torch.equal(grad_1, grad_0)
  assert torch.equal(lad_1[0], lad_0[0]) and torch.equal(lad_1[3], lad_0[3])


@pytest.mark.parametrize('n', EQUAL_N)
def test_lbfgs_with_and_without_the_ladder(ext, monkeypatch, n):
  """Ten iterations wired as train_gp wires them: the accepted row's (L,
  info, z) out of the 12-row ladder gives the bits a fresh factorisation of
  the 3 accepted rows gives."""
  set_mode(monkeypatch, None)
  raw, x, y = on_gpu(equal_case(n))

  def loss_fn(r):
    return gp_model.negative_log_marginal_likelihood(r, x, y)

  def vag(r, hint=None):
    return gp_model.nll_value_and_grad(r, x, y, chol_hint=hint)

  def ladder(r):
    nll_v, L, info, z = gp_model.nll_values_with_chol_z(r, x, y)
    return nll_v, (L, info, z)

  best_l, f_l = lbfgs.minimize_batched(
      loss_fn, raw.clone(), max_iters=10, check_every=5,
      value_and_grad_fn=vag, ladder_fn=ladder)
  best_0, f_0 = lbfgs.minimize_batched(
      loss_fn, raw.clone(), max_iters=10, check_every=5,
      value_and_grad_fn=vag, ladder_fn=None)
  f_start = gp_model.negative_log_marginal_likelihood(raw, x, y)
  print(f'OBSERVED lbfgs n={n}: f {f_start.tolist()} -> {f_0.tolist()}')
  assert bool(torch.isfinite(f_0).all()) and bool((f_0 < f_start).all())
  assert torch.equal(f_l, f_0)
  assert torch.equal(best_l, best_0)


# -- D: failed factorisations stay in their row --------------------------------------------


def check_failed_rows(case, run):
  """isinf(nll_r) == (info_r != 0) == (grad_r == 0).all() on every route."""
  failed = (run.info != 0)
  for route, (nll, grad) in run.routes.items():
    assert torch.equal(torch.isinf(nll), failed), (case.name, route)
    assert bool((nll[failed] > 0).all()), (case.name, route)
    if grad is not None:
      assert torch.equal((grad == 0).all(-1), failed), (case.name, route)
  assert torch.equal(torch.isinf(run.nll), failed), case.name


@pytest.mark.parametrize('n', fc.NAN_N)
def test_nan_amplitude_stays_in_its_row(ext, monkeypatch, n):
  """raw[1, 0] = NaN: K_1 is all NaN and every pivot test is `piv > 0`."""
  case = fc.nan_case(n)
  run = run_of(ext, monkeypatch, case)
  print(f'OBSERVED {case.name}: info {run.info.tolist()}')
  assert run.info[[0, 2]].tolist() == [0, 0] and int(run.info[1]) != 0
  assert bool(torch.isnan(run.K[1]).all())
  assert float(run.nll[1]) == math.inf
  for route, (nll, grad) in run.routes.items():
    assert float(nll[1]) == math.inf, route
    if grad is not None:
      assert bool((grad[1] == 0).all()), route
  check_failed_rows(case, run)
  check_factor_solve_nll(case, run)
  check_group(case.name, route_worsts([case], [run]),
              fc.cpu_group_worst(*fc.NAN_GROUP))


def test_near_singular_row_stays_in_its_row(ext, monkeypatch):
  """Eight duplicate row pairs and restart 1 at the noise floor. Whether
  restart 1 fails is rounding luck and not asserted; what it returns must be
  consistent with its info, and restarts 0 and 2 are held to A and, as a
  group over the four sizes, to B."""
  cases = [fc.make_dup_case(n) for n in fc.DUP_N]
  runs = [run_of(ext, monkeypatch, c) for c in cases]
  for case, run in zip(cases, runs):
    print(f'OBSERVED {case.name}: info {run.info.tolist()}, nll '
          f'{run.nll.tolist()}')
    check_failed_rows(case, run)
    check_factor_solve_nll(case, run)
  check_group('dup', route_worsts(cases, runs), fc.cpu_dup_worst())


# -- E: the gates ---------------------------------------------------------------------------


class Recorder:
  """The extension with the same attributes, noting the names called (and
  the solve's variant argument)."""

  def __init__(self, ext):
    self._ext, self.calls, self.variants = ext, [], []

  def __getattr__(self, name):
    target = getattr(self._ext, name)
    if not callable(target):
      return target

    def call(*args, **kwargs):
      self.calls.append(name)
      if name == 'batched_trsv_lower':
        self.variants.append(args[2] if len(args) > 2 else
                             kwargs.get('variant', 0))
      return target(*args, **kwargs)
    return call


GRAM, POTRF, TRSV = ('gram_matern52_batched', 'batched_potrf',
                     'batched_trsv_lower')
# id: (environment, n, R, fp64, requires_grad, kernels that run in
# nll_values_with_chol_z, trsv variant).
GATES = {
    'default': ({}, 97, 2, False, False, [GRAM, POTRF, TRSV], 0),
    'default-R1': ({}, 97, 1, False, False, [GRAM], None),
    'n1024': ({}, 1024, 2, False, False, [GRAM, POTRF, TRSV], 0),
    'n1025': ({}, 1025, 2, False, False, [GRAM, TRSV], 0),
    'n1200': ({}, 1200, 2, False, False, [GRAM, TRSV], 0),
    'n1201': ({}, 1201, 2, False, False, [GRAM], None),
    'mode-trsv': ({'VIZIER_AMD_CUSTOM_CHOL': 'trsv'}, 97, 2, False, False,
                  [GRAM, TRSV], 0),
    'mode-0': ({'VIZIER_AMD_CUSTOM_CHOL': '0'}, 97, 2, False, False,
               [GRAM], None),
    'mode-nonsense': ({'VIZIER_AMD_CUSTOM_CHOL': 'nonsense'}, 97, 2, False,
                      False, [GRAM], None),
    'mode-1': ({'VIZIER_AMD_CUSTOM_CHOL': '1'}, 97, 2, False, False,
               [GRAM, POTRF, TRSV], 0),
    'mode-both': ({'VIZIER_AMD_CUSTOM_CHOL': 'both'}, 97, 2, False, False,
                  [GRAM, POTRF, TRSV], 0),
    'trsv-v1': ({'VIZIER_AMD_TRSV': 'v1'}, 97, 2, False, False,
                [GRAM, POTRF, TRSV], 1),
    'mode-trsv-v1': ({'VIZIER_AMD_CUSTOM_CHOL': 'trsv',
                      'VIZIER_AMD_TRSV': 'v1'}, 97, 2, False, False,
                     [GRAM, TRSV], 1),
    'fp64': ({}, 97, 2, True, False, [], None),
    'requires-grad': ({}, 97, 2, False, True, [], None),
}


@pytest.mark.parametrize('gate', GATES)
def test_gates(ext, monkeypatch, gate):
  """Which kernels a fit runs: the ladder call, the gradient evaluation
  without a hint (the HIP pair or torch), with the hint (L, info) (no
  factorisation; the HIP solve wherever either gate is open) and with (L,
  info, z) (no solve either where z is the HIP solve's). Every NLL within
  1e-3 relative of the oracle, so a gate that picks a path which then
  breaks is seen."""
  env, n, r, fp64, requires_grad, want, variant = GATES[gate]
  case = fc.make_gate_case(n, r)
  nll64 = fc.oracle_nll(case)
  set_mode(monkeypatch, None)
  for key, value in env.items():
    monkeypatch.setenv(key, value)
  raw, x, y = on_gpu(case)
  if fp64:
    raw, x, y = raw.double(), x.double(), y.double()
  raw.requires_grad_(requires_grad)

  def recorded(fn):
    rec = Recorder(ext)
    with monkeypatch.context() as m:
      m.setattr(gp_model.ops, 'require_ext', lambda: rec)
      return rec, fn()

  def check_nll(what, nll):
    nll = nll.detach().double().cpu()
    err = float(((nll - nll64).abs() / nll64.abs()).max())
    print(f'OBSERVED gate {gate} {what}: nll within {err:.3e} of the oracle')
    assert bool(torch.isfinite(nll).all()) and err <= 1e-3, (gate, what, err)

  hip_solve = TRSV in want
  rec, (nll, L, info, z) = recorded(
      lambda: gp_model.nll_values_with_chol_z(raw, x, y))
  assert rec.calls == want, (gate, rec.calls)
  assert rec.variants == ([variant] if hip_solve else []), rec.variants
  assert tuple(z.shape) == ((r, n) if hip_solve else (r, n, 1))
  assert info.tolist() == [0] * r
  check_nll('ladder', nll)
  if requires_grad:
    # The autograd route: the loss is differentiable through the torch ops.
    grad, = torch.autograd.grad(nll.sum(), raw)
    assert bool(torch.isfinite(grad).all())
    return

  # The fused gram has no R condition of its own. Without a hint the
  # gradient evaluation runs the HIP solve only after the HIP factorisation:
  # the `trsv`-only composition exists on the ladder and hint paths alone.
  gram = [] if fp64 else [GRAM]
  both = want[1:] if POTRF in want else []
  rec, (nll_0, _) = recorded(lambda: gp_model.nll_value_and_grad(raw, x, y))
  assert rec.calls == gram + both, (gate, rec.calls)
  assert rec.variants == ([variant] if both else [])
  check_nll('no hint', nll_0)
  rec, (nll_2, _) = recorded(lambda: gp_model.nll_value_and_grad(
      raw, x, y, chol_hint=(L, info)))
  assert rec.calls == gram + ([TRSV] if hip_solve else []), (gate, rec.calls)
  assert rec.variants == ([variant] if hip_solve else [])
  check_nll('hint (L, info)', nll_2)
  rec, (nll_3, _) = recorded(lambda: gp_model.nll_value_and_grad(
      raw, x, y, chol_hint=(L, info, z)))
  assert rec.calls == gram, (gate, rec.calls)
  check_nll('hint (L, info, z)', nll_3)
