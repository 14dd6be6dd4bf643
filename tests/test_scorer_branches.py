"""Every kernel sequence of the fused posterior scorers, on synthetic operands.

Each binding in module.cpp picks a kernel sequence from (b, n) and two
environment switches. The operands come from tests/scorer_cases.py (no
fitted GP, no cancellation), every compare is against its fp64 reference,
and mean and quad = amp^2 - sd^2 are compared separately.

Branch -> cases (b, n, d); run for posterior_scores_chunked,
posterior_mean_std and posterior_scores_bf16:

  tile quadform, b <= 32, n < 4096     (1,63,1) (9,64,3) (25,200,10)
    ps_kvec[_bf16] + vz_quadform_tile    (32,257,13) (32,128,5)
  legacy chunked, b > 32, n < 4096     (33,257,13) scalar loads
    ps_kvec[_bf16] + ps_quadform         (40,260,7) float4 loads
    (NCHUNK = 10) + ps_finalize[_meanstd] (33,7,2) n < NCHUNK: empty chunks
  split + GEMM, n >= 4096              (25,4096,5) (1,4099,20) rchunks=512
    ps_kvec_split + ps_mu_dist_reduce    (32,4100,8) (33,4096,4) rchunks=15
    + rocBLAS + ps_finalize_*_direct
  posterior_mean_std_fp8               (9,64,3) (25,200,10)
    ps_kvec_fp8 + tile / GEMM            (32,257,40) dp=64, (25,4096,5)
  single-kernel posterior_scores       (1,63,1) (64,257,13) (5,4100,8)
  VIZIER_AMD_QUADFORM=custom (child A) (25,4096,5) (32,4100,8) (1,4099,20)
    ps_quadform_big                      + spikes at (25,4100,8)
  VIZIER_AMD_PS_GEMM_N=64 (child B),   (25,65,3) n<256, ichunks>n
    with and without QUADFORM=custom     (1,300,10) n<rchunks, (32,257,13)

Spikes (alpha = e_i, M = c e_i e_j^T; a dropped row, chunk or tile reads 0
instead of O(1)) run at (25,200,10), (33,257,13), (25,4100,8); the six
acquisition codes at (25,200,10), (33,257,13), (25,4096,5); the
trust-region mask on scorer_cases.TR_CASES (tile, legacy, split; nearest
row first, last and on a chunk boundary).

Bounds (scorer_cases.TOL_*): fp32 paths 2e-5 amp^2 = 3.38e-5 on mean and
on quad; codes 0,1,2,4,5 4e-5 amp; PI 1e-4; spikes 1e-5 relative; bf16 and
fp8 8x the error of the CPU fp32 torch emulation of the rounded-operand
formula, floored at 2e-5 amp^2. Measured emulation errors (mean, quad),
largest over all shapes above: bf16 (1.1e-6, 1.9e-7), fp8 (1.0e-6,
2.2e-7); so the floor, 3.38e-5, is the bound at every shape.

Largest error observed on the MI355X per branch (mean, quad), next to its
bound; `pytest -rA` prints the figure of every case (OBSERVED lines):

  tile      fp32 (4.3e-7, 1.7e-7)  bf16 (3.0e-7, 2.0e-7)    bound 3.38e-5
  legacy    fp32 (3.1e-7, 2.5e-7)  bf16 (2.9e-7, 2.0e-7)    bound 3.38e-5
  split     fp32 (3.5e-7, 1.6e-7)  bf16 (2.9e-7, 1.8e-7)    bound 3.38e-5
  fp8       (3.4e-7, 2.0e-7)                                bound 3.38e-5
  single    (4.4e-7, 1.7e-7)                                bound 3.38e-5
  child A   fp32 (3.5e-7, 1.8e-7)  bf16 (2.9e-7, 1.5e-7)
            fp8 (5.1e-7, 1.6e-7)                            bound 3.38e-5
  child B   gemm (3.0e-7, 1.9e-7)  custom (3.0e-7, 1.6e-7)
            fp8 (4.8e-7, 1.7e-7)                            bound 3.38e-5
  spikes    k_i 2.0e-7, c k_i k_j 6.8e-7 (relative)         bound 1e-5
  codes     0,1,2,4,5: 4.6e-7 (bound 5.2e-5)   PI: 2.0e-7 (bound 1e-4)
  trust region, unpenalised UCB: 4.2e-7                     bound 5.2e-5
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scorer_cases as sc

pytestmark = pytest.mark.gpu

_TESTS = os.path.dirname(os.path.abspath(__file__))
_REPO = os.path.dirname(_TESTS)


@pytest.fixture(scope='module')
def ext():
  from vizier_amd._src.ops import dispatch
  e = dispatch.require_ext()  # Fails loudly if the .so is missing.
  return e


_OPS = {}


def _ops(case_fn, *key) -> sc.Operands:
  """Device operands of a case: uploaded once, shared, never mutated."""
  if (case_fn, key) not in _OPS:
    _OPS[(case_fn, key)] = sc.Operands(case_fn(*key), 'cuda')
  return _OPS[(case_fn, key)]


def _report(what, err, tol):
  print(f'OBSERVED {what}: err {err:.3e} bound {tol:.3e}')


def _lowp(binding, ops):
  kind = sc.lowp_kind(binding)
  return None if kind is None else ops.lowp_operands(kind)


def _check_mean_sd(tag, case, binding, mean, sd, lo=None):
  e_mean, e_quad, tol_m, tol_q, emu = sc.errors_vs_reference(
      case, binding, mean, sd, lo)
  if emu is not None:
    print(f'EMULATION {tag}: mean {emu[0]:.3e} quad {emu[1]:.3e}')
  _report(f'{tag} mean', e_mean, tol_m)
  _report(f'{tag} quad', e_quad, tol_q)
  assert e_mean <= tol_m, f'{tag}: mean err {e_mean:.3e} > {tol_m:.3e}'
  assert e_quad <= tol_q, f'{tag}: quad err {e_quad:.3e} > {tol_q:.3e}'


def _ids(shapes):
  return ['-'.join(str(v) for v in s) for s in shapes]


# -- branch matrix ------------------------------------------------------------


@pytest.mark.parametrize('binding', ['chunked', 'mean_std', 'bf16'])
@pytest.mark.parametrize('branch,b,n,d', sc.BRANCH_SHAPES,
                         ids=_ids(sc.BRANCH_SHAPES))
def test_branch_matrix(ext, binding, branch, b, n, d):
  ops = _ops(sc.dense_case, b, n, d)
  mean, sd, dist = sc.mean_sd_dist(ext, binding, ops)
  _check_mean_sd(f'{binding} {branch} {(b, n, d)}', ops.case, binding,
                 mean, sd, _lowp(binding, ops))
  if dist is not None:
    want = sc.dense_reference(b, n, d).dist
    assert float((dist.cpu().double() - want).abs().max()) <= 1e-7


@pytest.mark.parametrize('b,n,d', sc.FP8_SHAPES, ids=_ids(sc.FP8_SHAPES))
def test_fp8_mean_std(ext, b, n, d):
  ops = _ops(sc.dense_case, b, n, d)
  mean, sd, dist = sc.mean_sd_dist(ext, 'fp8', ops)
  _check_mean_sd(f'fp8 {(b, n, d)}', ops.case, 'fp8', mean, sd,
                 _lowp('fp8', ops))
  want = sc.dense_reference(b, n, d).dist
  assert float((dist.cpu().double() - want).abs().max()) <= 1e-7


@pytest.mark.parametrize('b,n,d', sc.SINGLE_SHAPES,
                         ids=_ids(sc.SINGLE_SHAPES))
def test_single_kernel(ext, b, n, d):
  ops = _ops(sc.dense_case, b, n, d)
  mean, sd, _ = sc.mean_sd_dist(ext, 'single', ops)
  _check_mean_sd(f'single {(b, n, d)}', ops.case, 'single', mean, sd)


# -- spikes ---------------------------------------------------------------------

_SPIKE_RUNS = ([(bd,) + s for bd in ('chunked', 'mean_std')
                for s in sc.SPIKE_SHAPES] +
               [('bf16',) + sc.SPIKE_SHAPES[0],
                ('fp8',) + sc.SPIKE_SHAPES[0]])


@pytest.mark.parametrize('binding,path,b,n,d', _SPIKE_RUNS,
                         ids=_ids(_SPIKE_RUNS))
def test_spikes(ext, binding, path, b, n, d):
  ops = _ops(sc.dense_case, b, n, d)
  pairs = sc.spike_pairs(b, n, path)
  means, sds = sc.run_spikes(
      lambda alpha, M: sc.mean_sd_dist(ext, binding, ops, alpha=alpha,
                                       M=M)[:2], n, pairs, 'cuda')
  lo = _lowp(binding, ops)
  k = (sc.dense_reference(b, n, d).k if lo is None
       else sc.reference_lowp(ops.case, lo).k)
  e_mu, e_q = sc.spike_errors(k, pairs, means, sds)
  _report(f'spikes {binding} {path} k_i rel', float(e_mu.max()),
          sc.TOL_SPIKE_REL)
  _report(f'spikes {binding} {path} c*k_i*k_j rel', float(e_q.max()),
          sc.TOL_SPIKE_REL)
  bad_mu = [pairs[p] for p in
            torch.nonzero(e_mu.amax(1) > sc.TOL_SPIKE_REL).flatten()]
  bad_q = [pairs[p] for p in
           torch.nonzero(e_q.amax(1) > sc.TOL_SPIKE_REL).flatten()]
  assert not bad_mu, f'k_i wrong at spikes {bad_mu}'
  assert not bad_q, f'c*k_i*k_j wrong at spikes {bad_q}'


# -- acquisitions ---------------------------------------------------------------


@pytest.mark.parametrize('binding', ['chunked', 'bf16'])
@pytest.mark.parametrize('b,n,d', sc.ACQ_SHAPES, ids=_ids(sc.ACQ_SHAPES))
def test_acquisition_codes(ext, binding, b, n, d):
  ops = _ops(sc.dense_case, b, n, d)
  lo = _lowp(binding, ops)
  if lo is None:
    ref, scale = sc.dense_reference(b, n, d), 1.0
  else:
    ref, tol_m, tol_q, _ = sc.lowp_bounds(ops.case, lo)
    # The code bounds are derived from the mean/quad bound; they move
    # with it when the emulation lifts it off its floor.
    scale = max(tol_m, tol_q) / sc.TOL_FP32
  # The median of the reference mean: EI and PI see both signs of z.
  best = float(ref.mean.median()) if b > 1 else float(ref.mean[0])
  z = (ref.mean - best) / ref.sd
  assert float(z.min()) < 0 < float(z.max())
  for code, name in enumerate(sc.ACQ_NAMES):
    got = sc.scores(ext, binding, ops, code, coef=sc.COEF, best=best)
    want = sc.acquisition(code, ref.mean, ref.sd, sc.COEF, best)
    err = float((got.cpu().double() - want).abs().max())
    tol = sc.acq_tolerance(code) * scale
    _report(f'acq {binding} {(b, n, d)} {name}', err, tol)
    assert err <= tol, f'{name}: err {err:.3e} > {tol:.3e}'


# -- trust region and mask --------------------------------------------------------


@pytest.mark.parametrize('branch,b,n,nearest', sc.TR_CASES,
                         ids=_ids(sc.TR_CASES))
def test_trust_region_mask(ext, branch, b, n, nearest):
  ops = _ops(sc.tr_case, b, n, nearest)
  case = ops.case
  onehot = torch.tensor(sc.TR_ONEHOT, dtype=torch.uint8, device='cuda')
  keep = ~torch.tensor(sc.TR_ONEHOT, dtype=torch.bool)
  want_dist32 = (case.xq[:, None] - case.x)[..., keep].abs().amax(
      -1).amin(-1)
  ref = sc.reference(case, sc.TR_ONEHOT)
  h = b // 2
  # By construction: group 1 inside, group 2 outside the radius.
  assert float((ref.dist[:h] - sc.TR_NEAR).abs().max()) < 1e-6
  assert float((ref.dist[h:] - sc.TR_FAR).abs().max()) < 1e-6
  for binding in ('mean_std', 'fp8'):
    _, _, dist = sc.mean_sd_dist(ext, binding, ops, onehot=onehot)
    err = float((dist.cpu() - want_dist32).abs().max())
    assert err <= 1e-7, f'{binding} dist err {err:.3e}'
  for binding in ('chunked', 'bf16'):
    lo = _lowp(binding, ops)
    r = ref if lo is None else sc.reference_lowp(case, lo)
    ucb = sc.acquisition(0, r.mean, r.sd, sc.COEF, 0.0)
    for radius in (sc.TR_RADIUS, 0.0, 0.7):
      got = sc.scores(ext, binding, ops, 0, coef=sc.COEF,
                      tr_radius=radius, onehot=onehot).cpu().double()
      inside = slice(0, h) if radius == sc.TR_RADIUS else slice(0, b)
      err = float((got[inside] - ucb[inside]).abs().max())
      _report(f'tr {binding} {branch} r={radius} unpenalised', err,
              sc.TOL_ACQ)
      assert err <= sc.TOL_ACQ, (binding, radius, err)
      if radius == sc.TR_RADIUS:
        want = -1e4 - ref.dist[h:]
        err = float((got[h:] - want).abs().max())
        assert err <= sc.TOL_PENALTY, (binding, radius, err)


# -- hv_scalarize_tr --------------------------------------------------------------


@pytest.mark.parametrize('b', [1, 33])
@pytest.mark.parametrize('s', [1, 255, 256, 257, 1000])
@pytest.mark.parametrize('m', [1, 2, 3])
def test_hv_scalarize_tr(ext, m, s, b):
  g = torch.Generator().manual_seed(100 * m + s + b)

  def r(*shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64).float()
  # Every term positive: the mean over s has no cancellation, so
  # max|want| is the scale of every element.
  means, sds = 1.0 + r(m, b), 0.5 + r(m, b)
  weights = 0.2 + 0.8 * r(s, m)
  ref = 0.5 * r(m)
  dist = torch.where(torch.arange(b) % 2 == 0, sc.TR_NEAR, sc.TR_FAR)
  dist = dist.float()
  ucb = means.double() + sc.COEF * sds.double()
  for use_ref in (False, True):
    y = ucb - ref.double()[:, None] if use_ref else ucb
    want = (y[None] / weights.double()[:, :, None]).amin(1).mean(0)
    for use_dist in (False, True):
      got = ext.hv_scalarize_tr(
          means.cuda(), sds.cuda(), weights.cuda(),
          ref.cuda() if use_ref else None,
          dist.cuda() if use_dist else None, sc.COEF,
          sc.TR_RADIUS).cpu().double()
      out = dist > sc.TR_RADIUS if use_dist else torch.zeros(b).bool()
      tol = sc.TOL_HV_REL * float(want.abs().max())
      err = float((got - want)[~out].abs().max())
      assert err <= tol, (use_ref, use_dist, err, tol)
      if bool(out.any()):
        pen = -1e4 - dist.double()[out]
        assert float((got[out] - pen).abs().max()) <= sc.TOL_PENALTY


# -- argument checks ----------------------------------------------------------------


def _grow(t, dim=None):
  """`t` with one more element along `dim` (every dim when None)."""
  dims = range(t.dim()) if dim is None else [dim]
  shape = list(t.shape)
  for i in dims:
    shape[i] += 1
  out = torch.zeros(shape, dtype=t.dtype, device=t.device)
  out[tuple(slice(0, v) for v in t.shape)] = t
  return out


@pytest.mark.parametrize('binding',
                         ['chunked', 'bf16', 'mean_std', 'fp8'])
def test_scorer_argument_checks(ext, binding):
  """Wrong-shaped but LARGER operands: rejected on the host (the checks
  precede the first launch of each binding), harmless if they were not."""
  ops = _ops(sc.dense_case, 9, 64, 3)
  z2b, n2b = ops.bf16
  c = ops.fp8
  base = dict(xq=ops.xq, x=ops.x, ls=ops.ls, alpha=ops.alpha, M=ops.M,
              onehot=ops.onehot,
              z2=z2b if binding == 'bf16' else c.z2q,
              n2=n2b if binding == 'bf16' else c.n2)

  def call(a):
    if binding == 'chunked':
      return ext.posterior_scores_chunked(
          a['xq'], a['x'], a['ls'], sc.AMP, sc.MEAN_C, a['alpha'], a['M'],
          a['onehot'], 0, sc.COEF, 0.0, 0.0)
    if binding == 'bf16':
      return ext.posterior_scores_bf16(
          a['xq'], a['x'], a['z2'], a['n2'], a['ls'], sc.AMP, sc.MEAN_C,
          a['alpha'], a['M'], a['onehot'], 0, sc.COEF, 0.0, 0.0)
    if binding == 'mean_std':
      return ext.posterior_mean_std(
          a['xq'], a['x'], a['ls'], sc.AMP, sc.MEAN_C, a['alpha'], a['M'],
          a['onehot'])
    return ext.posterior_mean_std_fp8(
        a['xq'], a['x'], a['z2'], a['n2'], c.scale, a['ls'], sc.AMP,
        sc.MEAN_C, a['alpha'], a['M'], a['onehot'])

  call(base)  # the well-formed call is accepted
  wrong = {'x': _grow(ops.x, 1), 'ls': _grow(ops.ls),
           'alpha': _grow(ops.alpha), 'M': _grow(ops.M),
           'onehot': _grow(ops.onehot)}
  if binding in ('bf16', 'fp8'):
    wrong['z2'] = _grow(base['z2'], 0)
    wrong['n2'] = _grow(base['n2'])
  for name, value in wrong.items():
    with pytest.raises(RuntimeError):
      call(dict(base, **{name: value}))
  torch.cuda.synchronize()


def test_hv_scalarize_argument_checks(ext):
  m, b, s = 2, 5, 7
  means = torch.rand(m, b).cuda()
  sds = torch.rand(m, b).cuda() + 0.5
  weights = (0.2 + torch.rand(s, m)).cuda()
  ref, dist = torch.rand(m).cuda(), torch.rand(b).cuda()
  ext.hv_scalarize_tr(means, sds, weights, ref, dist, 1.8, 0.3)
  with pytest.raises(RuntimeError):
    ext.hv_scalarize_tr(means, _grow(sds, 1), weights, ref, dist, 1.8, 0.3)
  with pytest.raises(RuntimeError):
    ext.hv_scalarize_tr(means, sds, weights, _grow(ref), dist, 1.8, 0.3)
  with pytest.raises(RuntimeError):
    ext.hv_scalarize_tr(means, sds, weights, ref, _grow(dist), 1.8, 0.3)
  torch.cuda.synchronize()


# -- opt-in and threshold variants: one fresh child process each --------------------

_child_failed = []


def _run_child(tmp_path, switches, shapes, spikes=None):
  """Runs `python -m scorer_cases` with the given VIZIER_AMD_* switches
  (statics read once per process) and returns its outputs."""
  if _child_failed:
    pytest.fail(f'child {_child_failed[0]} failed earlier; '
                'not starting another')
  env = {k: v for k, v in os.environ.items()
         if k not in ('VIZIER_AMD_QUADFORM', 'VIZIER_AMD_PS_GEMM_N')}
  env.update(switches)
  env['PYTHONPATH'] = os.pathsep.join(
      [_REPO, _TESTS] + [p for p in [env.get('PYTHONPATH')] if p])
  out = tmp_path / 'child.npz'
  cmd = [sys.executable, '-m', 'scorer_cases', '--out', str(out),
         '--shapes', ';'.join(','.join(str(v) for v in s) for s in shapes)]
  if spikes is not None:
    cmd += ['--spikes', ','.join(str(v) for v in spikes)]
  try:
    res = subprocess.run(cmd, env=env, cwd=_REPO, capture_output=True,
                         text=True, timeout=120)
  except subprocess.TimeoutExpired:
    _child_failed.append(str(switches))
    pytest.fail(f'child {switches} timed out')
  if res.returncode != 0:
    _child_failed.append(str(switches))
    pytest.fail(f'child {switches} exited {res.returncode}:\n'
                f'{res.stderr[-2000:]}')
  return np.load(out)


def _check_child(tag, got, shapes):
  for shape in shapes:
    case = sc.dense_case(*shape)
    key = 'x'.join(str(v) for v in shape)
    for binding in sc.CHILD_BINDINGS:
      pre = f'{binding}/{key}'
      lo = None
      if sc.lowp_kind(binding) is not None:
        lo = {name: torch.from_numpy(got[f'{pre}/{name}'])
              for name in ('z1', 'z2', 'n2', 'scale')}
      _check_mean_sd(f'{tag} {binding} {shape}', case, binding,
                     got[f'{pre}/mean'], got[f'{pre}/sd'], lo)


def test_child_custom_quadform(ext, tmp_path):
  """VIZIER_AMD_QUADFORM=custom at n >= 4096: ps_quadform_big_kernel."""
  b, n, d = sc.CHILD_A_SPIKE_SHAPE
  got = _run_child(tmp_path, {'VIZIER_AMD_QUADFORM': 'custom'},
                   sc.CHILD_A_SHAPES, spikes=(b, n, d))
  _check_child('custom', got, sc.CHILD_A_SHAPES)
  pairs = sc.spike_pairs(b, n, 'custom')
  e_mu, e_q = sc.spike_errors(
      sc.dense_reference(b, n, d).k, pairs,
      torch.from_numpy(got['spikes/mean']),
      torch.from_numpy(got['spikes/sd']))
  _report('spikes custom k_i rel', float(e_mu.max()), sc.TOL_SPIKE_REL)
  _report('spikes custom c*k_i*k_j rel', float(e_q.max()),
          sc.TOL_SPIKE_REL)
  bad = [pairs[p] for p in torch.nonzero(
      (e_mu.amax(1) > sc.TOL_SPIKE_REL) |
      (e_q.amax(1) > sc.TOL_SPIKE_REL)).flatten()]
  assert not bad, f'wrong at spikes {bad}'


@pytest.mark.parametrize('quadform', ['gemm', 'custom'])
def test_child_low_gemm_threshold(ext, tmp_path, quadform):
  """VIZIER_AMD_PS_GEMM_N=64: the large-N code on its degenerate
  partitions (n < rchunks, ichunks > n, one partly filled j-chunk)."""
  switches = {'VIZIER_AMD_PS_GEMM_N': '64'}
  if quadform == 'custom':
    switches['VIZIER_AMD_QUADFORM'] = 'custom'
  got = _run_child(tmp_path, switches, sc.CHILD_B_SHAPES)
  _check_child(f'gemm_n=64/{quadform}', got, sc.CHILD_B_SHAPES)
