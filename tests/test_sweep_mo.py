"""The multi-objective sweep megakernel (eagle_sweep_mo.hip).

`ext.eagle_sweep_mo` is called directly on the adjusted steady-state pools
of tests/sweep_cases.py with M synthetic posteriors on one training set:

  one iteration   candidates against oracle.suggest; per metric k, mean and
                  quad from the kernel's own candidates within
                  scorer_cases.TOL_FP32; the distance bitwise; the score
                  against mean_s min_m (y_m - ref_m) / w[s, m] in float64
                  from the kernel's own mean and sd, within
                  4 (S + 4) 2^-24 mean_s |v_s| (one rounding each for the
                  UCB term, the subtraction, the quotient and the final
                  division, S for the sum; 4x as the other scorer tests)
  whole sweep     bitwise against eagle_suggest -> posterior_mean_std per
                  metric -> hv_scalarize_tr -> eagle_update, also at grids
                  1 and 7 (the launcher reads VIZIER_AMD_SWEEP_GRID on
                  every call)
  designers       same suggestions as under VIZIER_AMD_MEGAKERNEL_MO=0
  binding         every malformed operand raises
"""

import functools

import numpy as np
import pytest
import torch

import eagle_f64_oracle as oracle
import scorer_cases as sc
import sweep_cases as sw

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS = 2.0 ** -24
# id -> (pool, batch, dc, n, M, S); the README table says what each is the
# smallest case for.
CASES = {
    'base': (50, 25, 4, 63, 2, 7),
    'tile-64': (50, 25, 3, 64, 2, 7),
    'tile-65': (50, 25, 3, 65, 2, 7),
    'm-cap': (8, 4, 3, 70, 4, 300),
    'item-stride': (100, 25, 5, 600, 3, 16),
    'single-batch': (25, 25, 2, 130, 2, 7),
    'b1': (8, 1, 3, 70, 2, 1),
    'max-batch': (128, 32, 6, 200, 2, 7),
    'resident-cap': (128, 32, 32, 130, 2, 7),
    'w-cached': (8, 4, 3, 70, 3, 700),   # S * M > 2048: weights not in LDS
}
# Per metric: amplitude and mean constant, all different.
AMPS = [sc.AMP * r for r in (1.0, 0.9, 0.8, 0.7)]
MEAN_CS = [sc.MEAN_C + 0.1 * m for m in range(4)]
REF = [-0.5 - 0.1 * m for m in range(4)]   # below every y: no cancellation


@pytest.fixture(scope='module')
def ext():
  from vizier_amd._src.ops import dispatch
  return dispatch.require_ext()


@functools.lru_cache(maxsize=None)
def make(case_id, near=False):
  """The sweep case (state, x, metric 0) plus metrics 1 .. M - 1 and the
  weights. `near`: the half of the candidates with the smaller first
  coordinate get a training row each that differs from them in that
  coordinate only, by less than 0.3; it is more than 0.3 from the other
  half, and every other row is >= 1 from every candidate."""
  pool, batch, dc, n, m, s = CASES[case_id]
  seed = pool + 3 * dc + n
  case = sw.make_sweep_case(pool, batch, dc, n, seed, name=case_id)
  others = [sc.make_case(batch, n, dc, seed + 100 * i) for i in range(1, m)]
  case.m, case.s = m, s
  case.ls_m = [case.ls] + [o.ls for o in others]
  case.alpha_m = [case.alpha] + [o.alpha for o in others]
  case.M_m = [case.M] + [o.M for o in others]
  g = torch.Generator().manual_seed(seed)
  case.weights = (0.25 + 0.75 * torch.rand(s, m, generator=g)).float()
  if near:
    cand = sw.oracle_candidates(case)
    order = np.argsort(cand[:, 0])
    inside, mid = order[:batch // 2], cand[order[batch // 2 - 1:][:2], 0].mean()
    x = 2.0 + 0.5 * case.x.double().numpy()
    x[:batch // 2] = cand[inside]
    x[:batch // 2, 0] = mid - 0.3
    case.x = torch.from_numpy(x.astype(F32))
  return case


def call(case, iterations, ref=True, tr_radius=0.0):
  """The operands of ext.eagle_sweep_mo on fresh device copies, workspaces
  NaN; `.args()` is positional."""
  c = sw.sweep_call(case, iterations, tr_radius=tr_radius)
  m, b, n = case.m, case.batch, case.n

  def nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')
  c.ls_m = [t.cuda() for t in case.ls_m]
  c.inv_ls = torch.stack([1.0 / t for t in c.ls_m]).contiguous()
  c.alpha = torch.stack(case.alpha_m).cuda()
  c.kinv = [t.cuda() for t in case.M_m]
  c.amp2 = [a * a for a in AMPS[:m]]
  c.mean_c = MEAN_CS[:m]
  c.weights = case.weights.cuda()
  c.ref = torch.tensor(REF[:m]).cuda() if ref else None
  c.mask = torch.zeros(case.dc, dtype=torch.uint8, device='cuda')
  c.k_ws, c.mu_ws = nan(m, b, n), nan(m, b)
  c.var_ws, c.ms_ws, c.score_ws = nan(m, b, case.tiles + 1), nan(2, m, b), nan(b)
  cfg = oracle.Config()
  c.args = lambda: (
      c.pool_cont, c.rewards, c.perts, c.best, c.iter_t, c.barrier, c.x,
      c.inv_ls, c.alpha, c.kinv, c.amp2, c.mean_c, c.weights, c.ref, c.mask,
      c.out_cont, c.k_ws, c.mu_ws, c.dist_ws, c.var_ws, c.ms_ws, c.score_ws,
      c.n_batches, c.batch, c.pool, c.it_start, c.iterations, cfg.visibility,
      cfg.gravity, cfg.negative_gravity, cfg.normalization_scale,
      cfg.penalize_factor, cfg.perturbation_lower_bound, cfg.perturbation,
      c.seed, c.seed_update, sc.COEF, c.tr_radius)
  return c


def run(ext, case, iterations, **kwargs):
  c = call(case, iterations, **kwargs)
  c.grid = ext.eagle_sweep_mo(*c.args())
  torch.cuda.synchronize()
  return c


def state_of(c):
  return [t.cpu() for t in c.state()]


def _report(what, err, tol):
  print(f'OBSERVED {what}: err {err:.3e} (bound {tol:.3e})')
  assert err <= tol, (what, err, tol)


ONE_ITERATION = [(c, True, 0.0) for c in CASES] + [
    ('base', False, 0.0), ('base', True, 0.3), ('base', False, 0.3),
    ('base', True, 0.6)]


@pytest.mark.parametrize(
    'case_id,ref,radius', ONE_ITERATION,
    ids=[f'{c}{"" if r else "-noref"}-tr{t}' for c, r, t in ONE_ITERATION])
def test_one_iteration_against_fp64(ext, case_id, ref, radius):
  case = make(case_id, near=radius > 0)
  got = run(ext, case, 1, ref=ref, tr_radius=radius)
  assert 1 <= got.grid <= 128
  b, T = case.batch, case.tiles
  out_cont = got.out_cont.cpu().numpy()

  c64 = sw.oracle_candidates(case, np.float64)
  c32 = sw.oracle_candidates(case, F32)
  floor = 8.0 * case.pool * EPS * (1.0 + float(np.abs(case.pool_cont).max()))
  _report(f'{case_id} candidates',
          float(np.abs(out_cont.astype(np.float64) - c64).max()),
          max(4.0 * float(np.abs(c32 - c64).max()), floor))

  # Scorer stages per metric, from the kernel's own candidates.
  xq, x = torch.from_numpy(out_cont).double(), case.x.double()
  mu, var = got.mu_ws.cpu().double(), got.var_ws.cpu().double()
  mean_sd = got.ms_ws.cpu()
  for m in range(case.m):
    amp2 = AMPS[m] * AMPS[m]
    k = sc.kvec_direct(xq, x, case.ls_m[m].double()) * (amp2 / sc.AMP2)
    quad = ((k @ case.M_m[m].double()) * k).sum(-1)
    tag = f'{case_id} metric {m}'
    _report(f'{tag} k', float((got.k_ws[m].cpu().double() - k).abs().max()),
            sc.TOL_FP32)
    _report(f'{tag} mean', float(
        (mu[m] + MEAN_CS[m] - (MEAN_CS[m] + k @ case.alpha_m[m].double())
         ).abs().max()), sc.TOL_FP32)
    _report(f'{tag} quad', float((var[m, :, T] - quad).abs().max()),
            sc.TOL_FP32)
    assert torch.equal(mean_sd[0, m],
                       got.mu_ws[m].cpu() + F32(MEAN_CS[m]))
    _report(f'{tag} sd', float(
        (mean_sd[1, m].double() - (amp2 - quad).sqrt()).abs().max()),
            sc.TOL_ACQ)
  dist32 = sw.dist_f32(out_cont, case.x.numpy())
  assert np.array_equal(got.dist_ws.cpu().numpy(), dist32)

  # The score, from the kernel's own mean and sd.
  y = mean_sd[0].double() + sc.COEF * mean_sd[1].double()       # (M, b)
  if ref:
    y = y - torch.tensor(REF[:case.m]).float().double()[:, None]
  v = (y.T[:, None, :] / case.weights.double()[None]).amin(-1)  # (b, S)
  want = v.mean(-1)
  tol = 4.0 * (case.s + 4) * EPS * v.abs().mean(-1)
  score = got.score_ws.cpu()
  cut = torch.from_numpy(dist32 > F32(radius)) if 0 < radius <= 0.5 else \
      torch.zeros(b, dtype=torch.bool)
  if radius > 0:
    # Half the candidates are near a training row, the others are not.
    assert (dist32 > 0.3).sum() == b - b // 2
    assert bool(cut.any()) == (radius <= 0.5) and not bool(cut.all())
  assert np.array_equal(score[cut].numpy(), F32(-1e4) - dist32[cut.numpy()])
  ratio = ((score.double() - want).abs() / tol)[~cut]
  print(f'OBSERVED {case_id} score: worst err / bound {float(ratio.max()):.3f}')
  assert float(ratio.max()) <= 1.0
  assert got.iter_t[:2].tolist() == [case.it_start + 1, case.it_start]


def compose(ext, case, iterations, tr_radius):
  """The same iterations on the standalone step path, as the strategy and
  the designers' fused multi-objective closure make them."""
  c = call(case, iterations, tr_radius=tr_radius)
  pool3 = c.pool_cont.view(case.pool, 1, case.dc)
  pool_cat = torch.zeros(case.pool, 1, 0, dtype=torch.long, device='cuda')
  sizes = torch.zeros(0, dtype=torch.long, device='cuda')
  out_cont = torch.empty(case.batch, 1, case.dc, device='cuda')
  out_cat = torch.zeros(case.batch, 1, 0, dtype=torch.long, device='cuda')
  c.iter_t[:2] = case.it_start
  cfg = oracle.Config()
  for _ in range(iterations):
    ext.eagle_suggest(
        pool3, pool_cat, c.rewards, c.perts, sizes, c.iter_t, case.n_batches,
        case.batch, cfg.visibility, cfg.gravity, cfg.negative_gravity,
        cfg.normalization_scale, cfg.cat_factor, cfg.p_same, case.seed,
        out_cont, out_cat, 0)
    means, sds = [], []
    for m in range(case.m):
      mean, sd, dist = ext.posterior_mean_std(
          out_cont[:, 0, :], c.x, c.ls_m[m], AMPS[m], MEAN_CS[m], c.alpha[m],
          c.kinv[m], c.mask)
      means.append(mean)
      sds.append(sd)
    scores = ext.hv_scalarize_tr(torch.stack(means), torch.stack(sds),
                                 c.weights, c.ref, dist, sc.COEF, tr_radius)
    ext.eagle_update(
        pool3, pool_cat, c.rewards, c.perts, out_cont, out_cat, scores, sizes,
        c.best, c.iter_t, case.n_batches, cfg.penalize_factor,
        cfg.perturbation_lower_bound, cfg.perturbation, case.seed_update)
  torch.cuda.synchronize()
  return c


SWEEPS = [(c, 0) for c in CASES] + [('base', 1), ('base', 7)]


@pytest.mark.parametrize('case_id,grid', SWEEPS,
                         ids=[f'{c}-grid{g}' for c, g in SWEEPS])
def test_sweep_equals_step_kernels(ext, monkeypatch, case_id, grid):
  """2 n_batches + 1 iterations under a trust region that cuts some
  candidates off: the whole final state is bit-equal to the step path."""
  if grid:
    monkeypatch.setenv('VIZIER_AMD_SWEEP_GRID', str(grid))
  case = make(case_id)
  its = case.full_iterations()
  want = state_of(compose(ext, case, its, sc.TR_RADIUS))
  got = run(ext, case, its, tr_radius=sc.TR_RADIUS)
  assert got.grid == grid or not grid
  for g, w in zip(state_of(got), want):
    assert torch.equal(g, w)
  last = case.it_start + its - 1
  assert got.iter_t[:2].tolist() == [last + 1, last]
  assert not np.array_equal(want[1].numpy(), case.rewards)


def _designer(kind, extra, categorical):
  from vizier_amd import pyvizier as vz
  from vizier_amd._src.algorithms.core.abstractions import (
      ActiveTrials, CompletedTrials)
  from vizier_amd._src.algorithms.designers import gp_bandit, gp_ucb_pe
  problem = vz.ProblemStatement()
  for i in range(3):
    problem.search_space.root.add_float_param(f'x{i}', 0.0, 1.0)
  if categorical:
    problem.search_space.root.add_categorical_param('c', ['a', 'b'])
  problem.metric_information = vz.MetricsConfig([
      vz.MetricInformation(name=n, goal=vz.ObjectiveMetricGoal.MAXIMIZE)
      for n in ('f1', 'f2')])
  common = dict(max_evaluations=1500, ard_restarts=1, ard_max_iters=5,
                device='cuda', **extra)
  if kind == 'bandit':
    designer = gp_bandit.VizierGPBandit(
        problem, gp_bandit.GPBanditConfig(**common), seed=0)
  else:
    designer = gp_ucb_pe.VizierGPUCBPEBandit(
        problem, gp_ucb_pe.UCBPEConfig(
            pe_overwrite_probability=0.0, signal_to_noise_threshold=0.0,
            **common))   # the UCB phase, with certainty
  rng = np.random.default_rng(3)
  trials = []
  for uid in range(1, 41):
    x = rng.uniform(0, 1, 3)
    params = {f'x{i}': float(x[i]) for i in range(3)}
    if categorical:
      params['c'] = 'ab'[uid % 2]
    t = vz.Trial(params, id=uid)
    t.complete(vz.Measurement(metrics={
        'f1': float(-((x - 0.2) ** 2).sum()),
        'f2': float(-((x - 0.8) ** 2).sum())}))
    trials.append(t)
  designer.update(CompletedTrials(trials), ActiveTrials())
  return designer


@pytest.mark.parametrize('kind,extra,categorical,mega', [
    ('bandit', {}, False, True), ('ucb_pe', {}, False, True),
    ('bandit', {'scorer_gram_dtype': 'fp8'}, False, False),
    ('bandit', {}, True, False)],
    ids=['bandit', 'ucb-pe', 'fp8', 'categorical'])
def test_designer_suggestions_equal_hipgraph_path(monkeypatch, kind, extra,
                                                  categorical, mega):
  """A two-metric study on a continuous space takes the megakernel by
  default and suggests what the hipGraph path suggests; fp8 grams and a
  categorical parameter stay on the path they had."""
  out = {}
  for knob in ('1', '0'):
    monkeypatch.setenv('VIZIER_AMD_MEGAKERNEL_MO', knob)
    designer = _designer(kind, extra, categorical)
    out[knob] = designer.suggest(1)[0].parameters.as_dict()
    opt = designer._last_optimizer
    assert opt.last_used_megakernel == (mega and knob == '1')
    if mega:
      assert opt.last_graph_error is None
      assert opt.last_used_graph == (knob == '0')
  assert out['1'] == out['0']


def _grow(t, dim=-1):
  return torch.cat([t, t.narrow(dim, 0, 1)], dim).contiguous()


BAD = {
    'M = 1': lambda c: setattr(c, 'kinv', c.kinv[:1]),
    'M = 5': lambda c: setattr(c, 'kinv', (c.kinv * 3)[:5]),
    'n = 4096': lambda c: setattr(c, 'x', torch.zeros(4096, 4).cuda()),
    'amp2 length': lambda c: setattr(c, 'amp2', c.amp2[:1]),
    'inv_ls shape': lambda c: setattr(c, 'inv_ls', _grow(c.inv_ls)),
    'alpha shape': lambda c: setattr(c, 'alpha', _grow(c.alpha, 0)),
    'kinv shape': lambda c: setattr(c, 'kinv', [c.kinv[0], c.kinv[1][:-1]]),
    'weights metrics': lambda c: setattr(c, 'weights', _grow(c.weights)),
    'ref length': lambda c: setattr(c, 'ref', _grow(c.ref)),
    'mask length': lambda c: setattr(c, 'mask', c.mask[:-1]),
    'pool != n_batches * batch': lambda c: setattr(c, 'n_batches', 3),
    'k_ws small': lambda c: setattr(c, 'k_ws', c.k_ws[:1].contiguous()),
    'ms_ws small': lambda c: setattr(c, 'ms_ws', c.ms_ws[:1].contiguous()),
    'state not contiguous': lambda c: setattr(
        c, 'pool_cont', torch.zeros(4, 50).cuda().T),
}


@pytest.mark.parametrize('what', BAD)
def test_binding_rejects(ext, what):
  c = call(make('base'), 1)
  before = state_of(c)
  BAD[what](c)
  with pytest.raises(RuntimeError):
    ext.eagle_sweep_mo(*c.args())
  torch.cuda.synchronize()
  if what != 'state not contiguous':
    assert all(torch.equal(a, b) for a, b in zip(state_of(c), before))


def test_binding_resident_cap(ext):
  """pool * dc = 4096 runs (the 'resident-cap' case above); (128, 32, 33)
  is rejected before the launch."""
  pool, batch, dc, n, _, _ = CASES['resident-cap']
  assert pool * dc == 4096
  c = call(make('resident-cap'), 1)
  c.x = torch.zeros(n, dc + 1).cuda()
  with pytest.raises(RuntimeError, match='in LDS'):
    ext.eagle_sweep_mo(*c.args())
