"""The mixed-space sweep megakernel (eagle_sweep_mixed.hip).

`ext.eagle_sweep_mixed` is called directly on adjusted steady-state pools
(the construction of tests/sweep_cases.py: the visited rows get rewards far
outside the score range, so every row's kind is certain):

  one iteration   candidates against oracle.suggest (continuous within the
                  bound of test_sweep_kernel.py, categorical equal, every
                  entry's top-2 margin above tau), k / mean / quad / dist
                  from the kernel's own candidates decoded to dense, the
                  masked trust-region distance, and the update of both
                  halves of the state against oracle.update
  whole sweep     bitwise against eagle_suggest -> decode ->
                  posterior_scores_chunked -> eagle_update, in one launch,
                  in two, and at grids 1 and 7 (the mixed launcher reads
                  VIZIER_AMD_SWEEP_GRID on every call: no child process)
  designers       same suggestions as under VIZIER_AMD_MEGAKERNEL_MIXED=0
  binding         every malformed operand raises; the state is updated in
                  place
"""

import functools
import types

import numpy as np
import pytest
import torch

import eagle_f64_oracle as oracle
import scorer_cases as sc
import sweep_cases as sw

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS = 2.0 ** -24
SEED = sw.STRATEGY_SEED
CAT_CAP = 3072  # RESIDENT_CAT_CAP of eagle_sweep_common.h

# id -> (pool, batch, dc, cat sizes, n); the README table says what each
# is the smallest case for.
CASES = {
    'base': (50, 25, 3, (2, 5, 3), 63),
    'vec4': (50, 25, 2, (3, 3), 64),
    'pure-cat': (50, 25, 0, (4, 3, 2), 70),
    'wide': (32, 8, 1, (40,), 65),
    'many': (24, 8, 2, (2,) * (CAT_CAP // 24), 130),
    'b1': (8, 1, 2, (3,), 70),
    'max-batch': (128, 32, 4, (2, 3), 200),
    'unfolded': (50, 25, 3, (2, 3), 2049),
    'single-batch': (25, 25, 2, (3,), 130),
}
ROLES = ('low', 'dead', 'best', 'high')   # of visited row i: ROLES[i % 4]


@pytest.fixture(scope='module')
def ext():
  from vizier_amd._src.ops import dispatch
  return dispatch.require_ext()


def layout(dc, sizes):
  """Parameter order cat0, cont0, cat1, cont1, ...: (cont_cols, cat_start,
  D) with one-hot blocks and continuous columns interleaved."""
  cont_cols, cat_start, col = [], [], 0
  for i in range(max(dc, len(sizes))):
    if i < len(sizes):
      cat_start.append(col)
      col += sizes[i]
    if i < dc:
      cont_cols.append(col)
      col += 1
  return cont_cols, cat_start, col


def decode(case, cont, cat):
  """(B, dc), (B, dcat) -> dense (B, D), as EagleFeatureCodec.decode."""
  dense = np.zeros((cont.shape[0], case.d), dtype=F32)
  dense[:, case.cont_cols] = cont
  for j, start in enumerate(case.cat_start):
    dense[np.arange(cont.shape[0]), start + cat[:, j]] = 1.0
  return dense


@functools.lru_cache(maxsize=None)
def make(case_id, tr=False):
  pool, batch, dc, sizes, n = CASES[case_id]
  cont, cat, rewards, perts = oracle.steady_pool(
      pool, 1, dc, list(sizes), pool + 3 * dc + n)
  cont, rewards, perts = cont.astype(F32), rewards.astype(F32), \
      perts.astype(F32)
  cont_cols, cat_start, d = layout(dc, sizes)
  s = sc.make_case(batch, n, d, pool + n)
  n_batches = pool // batch
  it_start = 3 * n_batches - 1
  start = (it_start % n_batches) * batch
  for i in range(batch):
    role = ROLES[i % 4]
    rewards[start + i] = {'low': sw.LOW, 'best': sw.BEST}.get(
        role, sw.HIGH) + (0 if role == 'best' else sw.STEP * i)
    if role in ('dead', 'best'):
      perts[start + i] = sw.DEAD_PERT
  mask = np.zeros(d, dtype=np.uint8)
  for st, size in zip(cat_start, sizes):
    mask[st:st + size] = 1
  case = types.SimpleNamespace(
      name=case_id, pool=pool, batch=batch, dc=dc, sizes=list(sizes),
      dcat=len(sizes), n=n, d=d, cont_cols=cont_cols, cat_start=cat_start,
      mask=mask, cont=cont, cat=cat, rewards=rewards, perts=perts,
      best=F32(sw.BEST), n_batches=n_batches, it_start=it_start,
      start=start, x=s.x.clone(), ls=s.ls, alpha=s.alpha, M=s.M,
      tiles=((n + 63) // 64) ** 2,
      # 30 is the strategy's factor for a pure-categorical space.
      cfg=oracle.Config(cat_factor=30.0 if dc == 0 else 1.0))
  if tr:
    # Training row 0 equals candidate 0 but for its one-hot blocks (masked
    # columns only); every other row is >= 1 from every candidate.
    c64, k64, _ = suggest(case, np.float64)[:3]
    x = 2.0 + 0.5 * case.x.double().numpy()
    x[0] = decode(case, c64[:1].astype(F32),
                  (k64[:1] + 1) % np.array(sizes))[0]
    case.x = torch.from_numpy(x.astype(F32))
  return case


def suggest(case, arith):
  out = oracle.suggest(
      case.cont, case.cat, case.rewards, case.perts, case.sizes,
      case.it_start, case.n_batches, case.batch, SEED, case.cfg, dtype=F32,
      arith=arith, return_vals=True)
  return out[0][:, 0, :], out[1][:, 0, :], out[2], out[3]


def call(case, iterations, it_start=None, state=None, tr_radius=0.0,
         acq='ucb'):
  """The operands of ext.eagle_sweep_mixed on fresh device copies (or on
  `state`, an earlier call), workspaces NaN; `.args()` is positional."""
  from vizier_amd._src.ops import dispatch

  def dev(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).cuda()

  def nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')
  c = state or types.SimpleNamespace(
      pool_cont=dev(case.cont), pool_cat=dev(case.cat),
      rewards=dev(case.rewards), perts=dev(case.perts),
      best=dev([case.best]))
  c = types.SimpleNamespace(**vars(c))
  c.iter_t = torch.zeros(14, dtype=torch.long, device='cuda')
  c.barrier = torch.zeros(2, dtype=torch.int32, device='cuda')
  c.x, c.alpha, c.M = case.x.cuda(), case.alpha.cuda(), case.M.cuda()
  c.ls = case.ls.cuda()
  c.inv_ls = (1.0 / c.ls).contiguous()
  c.cat_sizes = dev(case.sizes, torch.int32)
  c.cont_cols = dev(case.cont_cols, torch.int32)
  c.cat_start = dev(case.cat_start, torch.int32)
  c.mask = dev(case.mask)
  c.out_cont = nan(case.batch, case.dc)
  c.out_cat = torch.full((case.batch, case.dcat), -1, dtype=torch.long,
                         device='cuda')
  c.k_ws, c.mu_ws = nan(case.batch, case.n), nan(case.batch)
  c.dist_ws, c.var_ws = nan(case.batch), nan(case.batch, case.tiles + 1)
  c.n_batches, c.batch, c.pool = case.n_batches, case.batch, case.pool
  c.it_start = case.it_start if it_start is None else it_start
  c.iterations, c.tr_radius = iterations, tr_radius
  c.acq = dispatch.ACQ_CODES[acq]
  cfg = case.cfg
  c.args = lambda: (
      c.pool_cont, c.pool_cat, c.rewards, c.perts, c.best, c.iter_t,
      c.barrier, c.x, c.inv_ls, c.alpha, c.M, c.cat_sizes, c.cont_cols,
      c.cat_start, c.mask, c.out_cont, c.out_cat, c.k_ws, c.mu_ws,
      c.dist_ws, c.var_ws, c.n_batches, c.batch, c.pool, c.it_start,
      c.iterations, cfg.visibility, cfg.gravity, cfg.negative_gravity,
      cfg.normalization_scale, cfg.cat_factor, cfg.p_same,
      cfg.penalize_factor, cfg.perturbation_lower_bound, cfg.perturbation,
      SEED, SEED ^ oracle.UPDATE_SEED_XOR, sc.AMP * sc.AMP, sc.MEAN_C,
      c.acq, sc.COEF, sw.BEST_VALUE, c.tr_radius)
  return c


def run(ext, case, iterations, **kwargs):
  c = call(case, iterations, **kwargs)
  c.grid = ext.eagle_sweep_mixed(*c.args())
  torch.cuda.synchronize()
  return c


def state_of(c):
  return [t.cpu() for t in (c.pool_cont, c.pool_cat, c.rewards, c.perts,
                            c.best)]


def _report(what, err, tol):
  print(f'OBSERVED {what}: err {err:.3e} (bound {tol:.3e})')
  assert err <= tol, (what, err, tol)


ONE_ITERATION = [(c, False) for c in CASES] + [('base', True)]


@pytest.mark.parametrize('case_id,tr', ONE_ITERATION,
                         ids=[c + ('-tr' if t else '')
                              for c, t in ONE_ITERATION])
def test_one_iteration_against_fp64(ext, case_id, tr):
  case = make(case_id, tr)
  tr_radius = sc.TR_RADIUS if tr else 0.0
  got = run(ext, case, 1, tr_radius=tr_radius)
  assert 1 <= got.grid <= 128
  start, batch, T = case.start, case.batch, case.tiles
  out_cont, out_cat = got.out_cont.cpu().numpy(), got.out_cat.cpu().numpy()

  # Candidates: continuous to tolerance, categorical equal, no entry left
  # out (every top-2 margin clears tau), and the mutation does mutate.
  c64, k64, margin, v64 = suggest(case, np.float64)
  c32, _, _, v32 = suggest(case, F32)
  if case.dc:
    floor = 8.0 * case.pool * EPS * (1.0 + float(np.abs(case.cont).max()))
    _report(f'{case_id} candidates',
            float(np.abs(out_cont.astype(np.float64) - c64).max()),
            max(4.0 * float(np.abs(c32 - c64).max()), floor))
  tau = 4.0 * float(np.nanmax(np.abs(v32 - v64)))
  print(f'OBSERVED {case_id}: smallest top-2 margin {margin:.3e} '
        f'(tau {tau:.3e})')
  assert margin > tau, (margin, tau)
  assert np.array_equal(out_cat, k64)
  changed = (k64 != case.cat[start:start + batch, 0, :]).mean()
  # Without forces an entry changes with probability 1 - p_same = 0.02;
  # half of that, where the case has entries enough to show it.
  if batch * case.dcat >= 64:
    assert changed >= 0.01, changed

  # Scorer stages from the kernel's own candidates, decoded to dense.
  xq32 = decode(case, out_cont, out_cat)
  xq, x = torch.from_numpy(xq32).double(), case.x.double()
  k = sc.kvec_direct(xq, x, case.ls.double())
  ref = sc.posterior_from_k(k, case.alpha.double(), case.M.double())
  _report(f'{case_id} k', float((got.k_ws.cpu().double() - k).abs().max()),
          sc.TOL_FP32)
  _report(f'{case_id} mean', float(
      (got.mu_ws.cpu().double() + sc.MEAN_C - ref.mean).abs().max()),
          sc.TOL_FP32)
  var = got.var_ws.cpu().double()
  _report(f'{case_id} quad', float((var[:, T] - ref.quad).abs().max()),
          sc.TOL_FP32)
  keep = case.mask == 0
  diff = np.abs(xq32[:, None, keep] - case.x.numpy()[None, :, keep])
  dist32 = diff.max(-1).min(-1) if case.dc else np.zeros(batch, F32)
  assert np.array_equal(got.dist_ws.cpu().numpy(), dist32)
  dist = torch.from_numpy(dist32).double()
  penalised = dist > tr_radius if tr else torch.zeros(batch, dtype=bool)
  if tr:
    assert not bool(penalised[0]) and bool(penalised[1:].any())
    unmasked = np.abs(xq32[:, None, :] - case.x.numpy()[None]).max(-1).min(-1)
    assert unmasked[0] == 1.0   # the nearest row differs in a one-hot column
  score = torch.where(penalised, -1e4 - dist, sc.acquisition(
      0, ref.mean, ref.sd, sc.COEF, sw.BEST_VALUE))

  # Update: kinds of all visited rows; both halves of the pool and the
  # perturbations bitwise (restarted rows are exact uniforms).
  post = oracle.update(
      case.cont, case.cat, case.rewards, case.perts, out_cont[:, None, :],
      out_cat[:, None, :], score.numpy(), case.sizes, float(case.best),
      case.it_start, case.n_batches, SEED ^ oracle.UPDATE_SEED_XOR, case.cfg,
      dtype=F32)
  cont, cat, rewards, perts, best = [t.numpy() for t in state_of(got)]
  kinds = post[5]
  want_kinds = [{'low': 'improved', 'dead': 'dead'}.get(
      ROLES[i % 4], 'penalised') for i in range(batch)]
  assert kinds == want_kinds
  assert np.array_equal(cont, post[0]) and np.array_equal(cat, post[1])
  assert np.array_equal(perts, post[3])
  accepted = np.zeros(case.pool, dtype=bool)
  accepted[start:start + batch] = [kd == 'improved' for kd in kinds]
  assert np.array_equal(rewards[~accepted], post[2][~accepted])
  tol = np.where(penalised.numpy(), sc.TOL_PENALTY, sc.acq_tolerance(0))
  err = np.abs(rewards[start:start + batch] - score.numpy())
  ok = ~accepted[start:start + batch] | (err <= tol)
  assert ok.all(), (err, tol)
  assert best[0] == case.best
  assert got.iter_t[:2].tolist() == [case.it_start + 1, case.it_start]


def compose(ext, case, iterations):
  """The same iterations on the standalone step path, as the strategy and
  the designers' score closure make them."""
  c = call(case, iterations)
  pool3 = c.pool_cont.view(case.pool, 1, case.dc)
  sizes = torch.tensor(case.sizes, dtype=torch.long, device='cuda')
  out_cont = torch.empty(case.batch, 1, case.dc, device='cuda')
  out_cat = torch.zeros(case.batch, 1, case.dcat, dtype=torch.long,
                        device='cuda')
  c.iter_t[:2] = case.it_start
  cfg, rows = case.cfg, torch.arange(case.batch, device='cuda')
  for _ in range(iterations):
    ext.eagle_suggest(
        pool3, c.pool_cat, c.rewards, c.perts, sizes, c.iter_t,
        case.n_batches, case.batch, cfg.visibility, cfg.gravity,
        cfg.negative_gravity, cfg.normalization_scale, cfg.cat_factor,
        cfg.p_same, SEED, out_cont, out_cat, max(case.sizes))
    dense = torch.zeros(case.batch, case.d, device='cuda')
    dense[:, case.cont_cols] = out_cont[:, 0, :]
    for j, st in enumerate(case.cat_start):
      dense[rows, st + out_cat[:, 0, j]] = 1.0
    scores = ext.posterior_scores_chunked(
        dense, c.x, c.ls, sc.AMP, sc.MEAN_C, c.alpha, c.M, c.mask, c.acq,
        sc.COEF, sw.BEST_VALUE, 0.0)
    ext.eagle_update(
        pool3, c.pool_cat, c.rewards, c.perts, out_cont, out_cat, scores,
        sizes, c.best, c.iter_t, case.n_batches, cfg.penalize_factor,
        cfg.perturbation_lower_bound, cfg.perturbation,
        SEED ^ oracle.UPDATE_SEED_XOR)
  torch.cuda.synchronize()
  return c


SWEEPS = [(c, 0) for c in CASES] + [('base', 1), ('base', 7)]


@pytest.mark.parametrize('case_id,grid', SWEEPS,
                         ids=[f'{c}-grid{g}' for c, g in SWEEPS])
def test_sweep_equals_step_kernels(ext, monkeypatch, case_id, grid):
  """2 n_batches + 1 iterations: the whole final state (continuous,
  categorical, rewards, perturbations, best_reward) is bit-equal to the
  step path, in one launch and across two launches that split them."""
  if grid:
    monkeypatch.setenv('VIZIER_AMD_SWEEP_GRID', str(grid))
  case = make(case_id)
  its = 2 * case.n_batches + 1
  want = state_of(compose(ext, case, its))
  one = run(ext, case, its)
  assert one.grid == grid or not grid
  first = run(ext, case, case.n_batches)
  two = run(ext, case, its - case.n_batches, state=first,
            it_start=case.it_start + case.n_batches)
  for got in (one, two):
    for g, w in zip(state_of(got), want):
      assert torch.equal(g, w)
    last = case.it_start + its - 1
    assert got.iter_t[:2].tolist() == [last + 1, last]
  # The run did move the state (restarts and the categorical mutation are
  # shown by the one-iteration test).
  assert not np.array_equal(want[2].numpy(), case.rewards)


def _designer(kind, acq, n_cat):
  from vizier_amd import pyvizier as vz
  from vizier_amd._src.algorithms.core.abstractions import (
      ActiveTrials, CompletedTrials)
  from vizier_amd._src.algorithms.designers import gp_bandit, gp_ucb_pe
  problem = vz.ProblemStatement()
  root = problem.search_space.root
  root.add_float_param('f0', -1.0, 1.0)
  root.add_categorical_param('c0', ['a', 'b', 'c'])
  if n_cat == 2:
    root.add_float_param('f1', 0.0, 4.0)
    root.add_int_param('i0', 1, 12)
  for j in range(1, n_cat):
    root.add_categorical_param(f'c{j}', ['u', 'v'])
  problem.metric_information.append(vz.MetricInformation(
      name='obj', goal=vz.ObjectiveMetricGoal.MAXIMIZE))
  common = dict(max_evaluations=1500, ard_restarts=1, ard_max_iters=5,
                device='cuda')
  if kind == 'bandit':
    designer = gp_bandit.VizierGPBandit(
        problem, gp_bandit.GPBanditConfig(acquisition=acq, **common))
  else:
    designer = gp_ucb_pe.VizierGPUCBPEBandit(
        problem, gp_ucb_pe.UCBPEConfig(
            pe_overwrite_probability=0.0, signal_to_noise_threshold=0.0,
            **common))   # the UCB phase, with certainty
  rng = np.random.default_rng(3)
  trials = []
  for uid in range(1, 41):
    params = {p.name: (float(rng.uniform(*p.bounds))
                       if p.type == vz.ParameterType.DOUBLE else
                       int(rng.integers(1, 13))
                       if p.type == vz.ParameterType.INTEGER else
                       str(rng.choice(p.feasible_values)))
              for p in problem.search_space.parameters}
    t = vz.Trial(params, id=uid)
    t.complete(vz.Measurement(metrics={'obj': float(
        -params['f0'] ** 2 + (params['c0'] == 'b'))}))
    trials.append(t)
  designer.update(CompletedTrials(trials), ActiveTrials())
  return designer


@pytest.mark.parametrize('kind,acq,n_cat', [
    ('bandit', 'ucb', 2), ('bandit', 'ei', 2), ('ucb_pe', 'ucb', 2),
    ('bandit', 'ucb', 33)], ids=['ucb', 'ei', 'ucb-pe', 'over-cat-cap'])
def test_designer_suggestions_equal_hipgraph_path(monkeypatch, kind, acq,
                                                  n_cat):
  """suggest() takes the mixed megakernel by default and returns what the
  hipGraph path returns; 33 categorical parameters on a pool of 100 pass
  the categorical resident cap and stay on the hipGraph path."""
  out = {}
  for mixed in ('1', '0'):
    monkeypatch.setenv('VIZIER_AMD_MEGAKERNEL_MIXED', mixed)
    designer = _designer(kind, acq, n_cat)
    out[mixed] = designer.suggest(1)[0].parameters.as_dict()
    opt = designer._last_optimizer
    assert opt.last_graph_error is None
    mega = mixed == '1' and n_cat == 2
    assert opt.last_used_megakernel == mega and opt.last_used_graph != mega
    if n_cat == 33:
      assert opt.strategy.pool_size * n_cat > CAT_CAP
  assert out['1'] == out['0']


BAD = {
    'D > 512': lambda c: setattr(c, 'x', torch.zeros(70, 513).cuda()),
    'Dc + sum != D': lambda c: setattr(
        c, 'cat_sizes', torch.tensor([2, 5, 4], dtype=torch.int32).cuda()),
    'Dcat < 1': lambda c: setattr(c, 'cat_sizes', c.cat_sizes[:0]),
    'size < 1': lambda c: setattr(
        c, 'cat_sizes', torch.tensor([0, 7, 3], dtype=torch.int32).cuda()),
    'column out of range': lambda c: c.cont_cols.fill_(13),
    'columns overlap': lambda c: c.cat_start.fill_(0),
    'int64 maps': lambda c: setattr(c, 'cat_start', c.cat_start.long()),
    'N > 8192': lambda c: setattr(c, 'x', torch.zeros(8193, 13).cuda()),
    'pool > 128': lambda c: setattr(c, 'pool', 129),
    'batch > 32': lambda c: setattr(c, 'batch', 33),
    'pool != n_batches * batch': lambda c: setattr(c, 'n_batches', 3),
    'mask length': lambda c: setattr(c, 'mask', c.mask[:5]),
    'pool_cat int32': lambda c: setattr(c, 'pool_cat', c.pool_cat.int()),
    'out_cat not contiguous': lambda c: setattr(
        c, 'out_cat', torch.zeros(3, 25, dtype=torch.long).cuda().T),
    'k_ws small': lambda c: setattr(c, 'k_ws', c.k_ws[:, :-1].contiguous()),
    'var_ws small': lambda c: setattr(c, 'var_ws', c.var_ws[:, :1]),
    'out_cat small': lambda c: setattr(c, 'out_cat', c.out_cat[:-1]),
    'iter_counter small': lambda c: setattr(c, 'iter_t', c.iter_t[:12]),
}


@pytest.mark.parametrize('what', BAD)
def test_binding_rejects(ext, what):
  c = call(make('base'), 1)
  before = state_of(c)
  BAD[what](c)
  with pytest.raises(RuntimeError):
    ext.eagle_sweep_mixed(*c.args())
  torch.cuda.synchronize()
  if what != 'pool_cat int32':
    assert all(torch.equal(a, b) for a, b in zip(state_of(c), before))


def test_binding_caps_and_in_place(ext):
  """pool * Dcat at the cap runs ('many'); one more categorical parameter
  is rejected, as is a continuous pool past RESIDENT_CAP. The state
  tensors are updated where they are."""
  case = make('many')
  assert case.pool * case.dcat == CAT_CAP
  c = call(case, 1)
  ptrs = [t.data_ptr() for t in (c.pool_cont, c.pool_cat, c.rewards,
                                 c.perts, c.best)]
  before = state_of(c)
  ext.eagle_sweep_mixed(*c.args())
  torch.cuda.synchronize()
  assert ptrs == [t.data_ptr() for t in (c.pool_cont, c.pool_cat, c.rewards,
                                         c.perts, c.best)]
  assert not any(torch.equal(a, b) for a, b in zip(state_of(c)[:4], before))
  pool, batch, dc, sizes, n = CASES['many']
  for dc2, sizes2 in ((dc, sizes + (2,)), (4096 // pool + 1, (2,))):
    cont_cols, cat_start, d = layout(dc2, sizes2)
    over = sc.make_case(batch, n, d, 1)
    big = types.SimpleNamespace(**{**vars(case), **dict(
        dc=dc2, sizes=list(sizes2), dcat=len(sizes2), d=d,
        cont_cols=cont_cols, cat_start=cat_start,
        mask=np.zeros(d, np.uint8), x=over.x, ls=over.ls,
        cont=np.zeros((pool, 1, dc2), F32),
        cat=np.zeros((pool, 1, len(sizes2)), np.int64))})
    with pytest.raises(RuntimeError, match='in LDS'):
      ext.eagle_sweep_mixed(*call(big, 1).args())
