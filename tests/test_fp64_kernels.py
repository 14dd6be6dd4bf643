"""The fp64 HIP kernels (VIZIER_AMD_FP64_HIP=1 path) against fp64 references.

  posterior_score_f64.hip  ps_kvec_f64 + ps_quadform_f64 (MFMA f64 16x16x4,
                           slabs, candidate tiles) + ps_finalize_f64
  gram_matern52_f64.hip    difference-form Gram / cross-Gram
  eagle_step.hip (double)  suggest / update against tests/eagle_f64_oracle.py,
                           at q = 1 and at q > 1

Scorer operands are the fp32-valued cases of tests/scorer_cases.py, so
`.double()` is exact and `reference(case)` is the exact-operand reference.

Bounds are derived, never measured (u = 2^-53):
  quad  8 n u (|k|^T |M| |k|), per candidate, from the reference's own k:
        the running error bound of an n-term double accumulation, doubled
        because the reference rounds too.
  mean  8 n u (|k| . |alpha|) + 2^-52 |MEAN_C|.
  k     amp^2 (d + 16) 2^-52 * 4 (Gram test). The CPU reference uses the
        n1 + n2 - 2 z1.z2 form; with x in [0, 1] and lengthscales >=
        sqrt(d) every norm is <= 1, so its cancellation error in d2 is
        <= ~2 (d + 2) u and |dk/dd2| <= 5/6 amp^2 keeps it inside the bound.
  codes |dmean| + coef |dsd| with dsd = dquad / (2 sd); PI 1e-12.
Every bound is asserted to be below 1e-3 * TOL_FP32, which also proves the
path under test is not the fp32 one. `pytest -rA` prints each figure.

Largest errors observed on the MI355X next to the smallest bound they were
held to (OBSERVED lines): scorer mean 3.6e-15 (bound 5.4e-13 .. 2.8e-10),
quad 3.3e-16 (4.1e-14 .. 1.3e-10), codes 1.6e-15 (4.8e-12), PI 6.7e-16
(1e-12), Gram 8.9e-16 (3.0e-14), Eagle suggest 4.4e-16 (8.8e-14).
"""

import math

import numpy as np
import pytest
import torch

import eagle_f64_oracle as oracle
import scorer_cases as sc

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
NOT_FP32 = 1e-3 * sc.TOL_FP32

SCORER_SHAPES = [(1, 63, 1), (9, 64, 3), (25, 200, 10), (32, 257, 13),
                 (33, 258, 7), (16, 16, 2), (5, 4100, 8)]
ACQ_SHAPES = [(25, 200, 10), (33, 257, 13)]
TR_SHAPES = [(24, 300, 0), (24, 300, 299), (24, 300, 256)]
GRAM_SHAPES = [(16, 16, 4), (100, 37, 20), (257, 513, 51)]


def _ids(shapes):
  return ['x'.join(str(v) for v in s) for s in shapes]


@pytest.fixture(scope='module')
def ext():
  from vizier_amd._src.ops import dispatch
  return dispatch.require_ext()  # Fails loudly if the .so is missing.


class Ops64:
  """A case's tensors as float64 on the GPU (exact images of the fp32)."""

  def __init__(self, case, onehot=None):
    self.case = case
    self.x = case.x.double().cuda()
    self.xq = case.xq.double().cuda()
    self.ls = case.ls.double().cuda()
    self.alpha = case.alpha.double().cuda()
    self.M = case.M.double().cuda()
    if onehot is None:
      onehot = [0] * case.d
    self.onehot = torch.tensor(onehot, dtype=torch.uint8, device='cuda')

  def mean_std(self, ext):
    return ext.posterior_mean_std_f64(
        self.xq, self.x, self.ls, sc.AMP, sc.MEAN_C, self.alpha, self.M,
        self.onehot)

  def scores(self, ext, code, coef=0.0, best=0.0, tr_radius=0.0):
    return ext.posterior_scores_f64(
        self.xq, self.x, self.ls, sc.AMP, sc.MEAN_C, self.alpha, self.M,
        self.onehot, code, coef, best, tr_radius)


def _bounds(case, ref):
  """Per-candidate (mean bound, quad bound) from the reference's own k."""
  k = ref.k.abs()
  quad = 8.0 * case.n * U * ((k @ case.M.double().abs()) * k).sum(-1)
  mean = (8.0 * case.n * U * (k @ case.alpha.double().abs()) +
          2.0 ** -52 * abs(sc.MEAN_C))
  assert float(quad.max()) < NOT_FP32 and float(mean.max()) < NOT_FP32
  return mean, quad


def _acq_bound(ref, tol_mean, tol_quad):
  return tol_mean + sc.COEF * tol_quad / (2.0 * ref.sd)


# -- scorer parts ---------------------------------------------------------------


@pytest.mark.parametrize('b,n,d', SCORER_SHAPES, ids=_ids(SCORER_SHAPES))
def test_scorer_parts(ext, b, n, d):
  case = sc.dense_case(b, n, d)
  ref = sc.dense_reference(b, n, d)
  tol_mean, tol_quad = _bounds(case, ref)
  mean, sd, dist = (t.cpu() for t in Ops64(case).mean_std(ext))
  assert mean.dtype == sd.dtype == dist.dtype == torch.float64
  e_mean = (mean - ref.mean).abs()
  e_quad = ((sc.AMP2 - sd * sd) - ref.quad).abs()
  print(f'OBSERVED parts {(b, n, d)}: mean {float(e_mean.max()):.3e} '
        f'(bound {float(tol_mean.max()):.3e}), quad '
        f'{float(e_quad.max()):.3e} (bound {float(tol_quad.max()):.3e})')
  assert bool((e_mean <= tol_mean).all()), (e_mean / tol_mean).max()
  assert bool((e_quad <= tol_quad).all()), (e_quad / tol_quad).max()
  assert torch.equal(dist, ref.dist)


def test_scorer_is_deterministic(ext):
  ops = Ops64(sc.dense_case(25, 200, 10))
  first, second = ops.mean_std(ext), ops.mean_std(ext)
  for a, b in zip(first, second):
    assert torch.equal(a, b)
  s1 = ops.scores(ext, 0, coef=sc.COEF)
  s2 = ops.scores(ext, 0, coef=sc.COEF)
  assert torch.equal(s1, s2)


@pytest.mark.parametrize('b,n,d', ACQ_SHAPES, ids=_ids(ACQ_SHAPES))
def test_acquisition_codes(ext, b, n, d):
  case = sc.dense_case(b, n, d)
  ref = sc.dense_reference(b, n, d)
  tol = _acq_bound(ref, *_bounds(case, ref))
  ops = Ops64(case)
  # The median of the reference mean: EI and PI see both signs of z.
  best = float(ref.mean.median())
  z = (ref.mean - best) / ref.sd
  assert float(z.min()) < 0 < float(z.max())
  for code, name in enumerate(sc.ACQ_NAMES):
    got = ops.scores(ext, code, coef=sc.COEF, best=best).cpu()
    want = sc.acquisition(code, ref.mean, ref.sd, sc.COEF, best)
    err = (got - want).abs()
    bound = torch.full_like(tol, 1e-12) if name == 'pi' else tol
    print(f'OBSERVED acq {(b, n, d)} {name}: {float(err.max()):.3e} '
          f'(bound {float(bound.max()):.3e})')
    assert bool((err <= bound).all()), (name, float((err / bound).max()))


@pytest.mark.parametrize('b,n,nearest', TR_SHAPES, ids=_ids(TR_SHAPES))
def test_trust_region_mask(ext, b, n, nearest):
  case = sc.tr_case(b, n, nearest)
  h = b // 2
  inverted = [1 - v for v in sc.TR_ONEHOT]
  plain = sc.reference(case, sc.TR_ONEHOT)
  tol = _acq_bound(plain, *_bounds(case, plain))
  ucb = sc.acquisition(0, plain.mean, plain.sd, sc.COEF, 0.0)
  # By construction: group 1 inside, group 2 outside the radius.
  assert float((plain.dist[:h] - sc.TR_NEAR).abs().max()) < 1e-6
  assert float((plain.dist[h:] - sc.TR_FAR).abs().max()) < 1e-6
  for onehot, inside, outside in (
      (sc.TR_ONEHOT, slice(0, h), slice(h, b)),
      (inverted, slice(h, b), slice(0, h))):
    ops = Ops64(case, onehot)
    dist = sc.reference(case, onehot).dist
    assert torch.equal(ops.mean_std(ext)[2].cpu(), dist)
    assert float(dist[inside].max()) < sc.TR_RADIUS < float(
        dist[outside].min())
    got = ops.scores(ext, 0, coef=sc.COEF, tr_radius=sc.TR_RADIUS).cpu()
    assert bool(((got[inside] - ucb[inside]).abs() <= tol[inside]).all())
    e_pen = (got[outside] - (-1e4 - dist[outside])).abs()
    assert float(e_pen.max()) <= 2.0 ** -52 * 1e4
    # Radius 0 and a radius above 0.5 both switch the penalty off.
    for radius in (0.0, 0.7):
      got = ops.scores(ext, 0, coef=sc.COEF, tr_radius=radius).cpu()
      assert bool(((got - ucb).abs() <= tol).all())


def test_argument_checks(ext):
  ops = Ops64(sc.dense_case(9, 64, 3))
  tail = (sc.AMP, sc.MEAN_C, ops.alpha, ops.M, ops.onehot)
  with pytest.raises(RuntimeError, match='fp64'):
    ext.posterior_scores_f64(ops.xq.float(), ops.x, ops.ls, *tail, 0,
                             sc.COEF, 0.0, 0.0)
  with pytest.raises(RuntimeError, match='fp64'):
    ext.posterior_mean_std_f64(ops.xq, ops.x, ops.ls, sc.AMP, sc.MEAN_C,
                               ops.alpha, ops.M.float(), ops.onehot)
  with pytest.raises(RuntimeError, match='fp64'):
    ext.gram_matern52_f64(ops.xq.float(), ops.x.float(), ops.ls.float(),
                          sc.AMP)
  short = ops.onehot[:-1].contiguous()
  with pytest.raises(RuntimeError, match='onehot'):
    ext.posterior_scores_f64(ops.xq, ops.x, ops.ls, sc.AMP, sc.MEAN_C,
                             ops.alpha, ops.M, short, 0, sc.COEF, 0.0, 0.0)
  with pytest.raises(RuntimeError, match='alpha'):
    ext.posterior_mean_std_f64(ops.xq, ops.x, ops.ls, sc.AMP, sc.MEAN_C,
                               ops.alpha[:-1].contiguous(), ops.M,
                               ops.onehot)


# -- gram ---------------------------------------------------------------------------


@pytest.mark.parametrize('n,m,d', GRAM_SHAPES, ids=_ids(GRAM_SHAPES))
def test_gram_f64(ext, n, m, d):
  from vizier_amd._src.gp import matern
  g = torch.Generator().manual_seed(31 * n + m + d)
  x1 = torch.rand(n, d, generator=g, dtype=torch.float64)
  x2 = torch.rand(m, d, generator=g, dtype=torch.float64)
  ls = math.sqrt(d) * (1.0 + torch.rand(d, generator=g,
                                        dtype=torch.float64))
  amp = torch.tensor(sc.AMP, dtype=torch.float64)
  bound = sc.AMP2 * (d + 16) * 2.0 ** -52 * 4
  assert bound < NOT_FP32
  want = matern.gram_matern52(x1, x2, ls, amp)
  x1g, x2g, lsg = x1.cuda(), x2.cuda(), ls.cuda()
  got = ext.gram_matern52_f64(x1g, x2g, lsg, sc.AMP).cpu()
  err = float((got - want).abs().max())
  print(f'OBSERVED gram {(n, m, d)}: {err:.3e} (bound {bound:.3e})')
  assert got.shape == (n, m) and err <= bound
  # Symmetric call: exactly symmetric, diagonal exactly amp^2.
  sym = ext.gram_matern52_f64(x1g, x1g, lsg, sc.AMP).cpu()
  assert torch.equal(sym, sym.T)
  assert torch.equal(sym.diagonal(),
                     torch.full((n,), sc.AMP * sc.AMP, dtype=torch.float64))
  want_sym = matern.gram_matern52(x1, None, ls, amp)
  assert float((sym - want_sym).abs().max()) <= bound


def test_gram_dispatch_under_flag(ext, monkeypatch):
  from vizier_amd._src.ops import dispatch
  g = torch.Generator().manual_seed(5)
  x1 = torch.rand(40, 6, generator=g, dtype=torch.float64).cuda()
  x2 = torch.rand(23, 6, generator=g, dtype=torch.float64).cuda()
  ls = (1.0 + torch.rand(6, generator=g, dtype=torch.float64)).cuda()
  amp = torch.tensor(sc.AMP, dtype=torch.float64, device='cuda')
  monkeypatch.setenv('VIZIER_AMD_FP64_HIP', '1')
  assert torch.equal(dispatch.gram_matern52(x1, x2, ls, amp),
                     ext.gram_matern52_f64(x1, x2, ls, sc.AMP))
  on = dispatch.gram_matern52(x1, None, ls, amp)
  assert torch.equal(on.diagonal(), torch.full_like(on.diagonal(),
                                                    sc.AMP * sc.AMP))


# -- eagle --------------------------------------------------------------------------


def _eagle_inputs(pool, dc, cat_sizes, seed, q=1):
  """A steady-state pool: a few -inf rewards, spread perturbations."""
  return oracle.steady_pool(pool, q, dc, cat_sizes, seed)


def _run_suggest(ext, pool_cont, pool_cat, rewards, perts, cat_sizes,
                 offset, n_batches, batch, seed, cfg):
  dev = 'cuda'
  q, dc, dcat = pool_cont.shape[1], pool_cont.shape[2], pool_cat.shape[2]
  iter_t = torch.zeros(12, dtype=torch.long, device=dev)
  iter_t[:2] = offset
  out_cont = torch.empty(batch, q, dc, dtype=torch.float64, device=dev)
  out_cat = torch.empty(batch, q, dcat, dtype=torch.long, device=dev)
  ext.eagle_suggest_f64(
      torch.from_numpy(pool_cont).to(dev), torch.from_numpy(pool_cat).to(dev),
      torch.from_numpy(rewards).to(dev), torch.from_numpy(perts).to(dev),
      torch.tensor(cat_sizes, dtype=torch.long, device=dev), iter_t,
      n_batches, batch, cfg.visibility, cfg.gravity, cfg.negative_gravity,
      cfg.normalization_scale, cfg.cat_factor, cfg.p_same, seed, out_cont,
      out_cat, max(cat_sizes, default=0))
  assert iter_t[:2].tolist() == [offset, offset]
  return out_cont.cpu().numpy(), out_cat.cpu().numpy()


@pytest.mark.parametrize('pool,batch,dc', [(50, 25, 4), (100, 25, 20)],
                         ids=['50x25x4', '100x25x20'])
def test_eagle_suggest_continuous(ext, pool, batch, dc):
  cfg = oracle.Config()
  seed, n_batches = 12345, pool // batch
  offset = n_batches + 3               # steady state, batch_start > 0
  inputs = _eagle_inputs(pool, dc, [], seed=pool + dc)
  want, _, _ = oracle.suggest(*inputs, [], offset, n_batches, batch, seed,
                              cfg)
  got, _ = _run_suggest(ext, *inputs, [], offset, n_batches, batch, seed,
                        cfg)
  tol = 8.0 * pool * U * (1.0 + float(np.abs(inputs[0]).max()))
  err = float(np.abs(got - want).max())
  print(f'OBSERVED suggest {(pool, batch, dc)}: {err:.3e} (bound {tol:.3e})')
  assert err <= tol


def _check_suggest_mixed(ext, q):
  cfg = oracle.Config()
  pool, batch, dc, cat_sizes = 50, 25, 3, [3, 5]
  seed, n_batches = 2024, 2
  offset = 5
  inputs = _eagle_inputs(pool, dc, cat_sizes, seed=77, q=q)
  want_cont, want_cat, margin = oracle.suggest(
      *inputs, cat_sizes, offset, n_batches, batch, seed, cfg)
  # Every top-2 `logit + gumbel` gap is far above rounding: the argmax is
  # unambiguous for this seed, for all 25 x 2 entries.
  assert margin > 1e-9, margin
  got_cont, got_cat = _run_suggest(ext, *inputs, cat_sizes, offset,
                                   n_batches, batch, seed, cfg)
  tol = 8.0 * pool * U * (1.0 + float(np.abs(inputs[0]).max()))
  assert float(np.abs(got_cont - want_cont).max()) <= tol
  assert np.array_equal(got_cat, want_cat)
  # The mutation moved some, not all, categories.
  start = (offset % n_batches) * batch
  changed = (want_cat != inputs[1][start:start + batch]).mean()
  assert 0.0 < changed < 1.0


def test_eagle_suggest_mixed(ext):
  _check_suggest_mixed(ext, q=1)


def test_eagle_suggest_mixed_q3(ext):
  # q > 1 (what acquisition='qei' runs): distances over the flat q * D
  # features, noise normalised over the q axis, draws indexed over q.
  _check_suggest_mixed(ext, q=3)


def test_eagle_suggest_continuous_q2(ext):
  cfg = oracle.Config()
  pool, batch, dc, seed, n_batches = 60, 20, 5, 12345, 3
  offset = 8                            # batch_start = 40
  inputs = _eagle_inputs(pool, dc, [], seed=pool + dc, q=2)
  want, _, _ = oracle.suggest(*inputs, [], offset, n_batches, batch, seed,
                              cfg)
  got, _ = _run_suggest(ext, *inputs, [], offset, n_batches, batch, seed,
                        cfg)
  tol = 8.0 * pool * U * (1.0 + float(np.abs(inputs[0]).max()))
  err = float(np.abs(got - want).max())
  print(f'OBSERVED suggest q2 {(pool, batch, dc)}: {err:.3e} '
        f'(bound {tol:.3e})')
  assert got.shape == (batch, 2, dc) and err <= tol


def test_eagle_update_bitwise(ext):
  _check_update_bitwise(ext, q=1)


def test_eagle_update_bitwise_q3(ext):
  _check_update_bitwise(ext, q=3)


def _check_update_bitwise(ext, q):
  cfg = oracle.Config()
  pool, batch, dc, cat_sizes = 50, 25, 3, [3, 5]
  strategy_seed, n_batches, offset = 99, 2, 5
  seed = strategy_seed ^ oracle.UPDATE_SEED_XOR
  start = (offset % n_batches) * batch
  rng = np.random.default_rng(8)
  pool_cont, pool_cat, rewards, perts = _eagle_inputs(pool, dc, cat_sizes,
                                                      seed=9, q=q)
  rewards[start:start + batch] = rng.normal(size=batch)
  batch_cont = rng.random((batch, q, dc))
  batch_cat = np.stack([rng.integers(0, s, size=(batch, q))
                        for s in cat_sizes], axis=-1).astype(np.int64)
  # Even rows improve, odd rows do not; rows 1 and 3 are one penalty away
  # from the lower bound (dead), row 4 improves but is already below it
  # (dead), and so is row 0, which becomes the new best (exempt).
  delta = np.where(np.arange(batch) % 2 == 0, 0.5, -0.5)
  delta[0] = 5.0
  batch_rewards = rewards[start:start + batch] + delta
  perts[start:start + batch] = 0.16
  perts[start + 1] = perts[start + 3] = 8e-5
  perts[start] = perts[start + 4] = 5e-5
  best = float(rewards[np.isfinite(rewards)].max())
  want = oracle.update(pool_cont, pool_cat, rewards, perts, batch_cont,
                       batch_cat, batch_rewards, cat_sizes, best, offset,
                       n_batches, seed, cfg)
  kinds = want[5]
  assert {'improved', 'penalised', 'dead'} == set(kinds)
  assert kinds[1] == kinds[3] == kinds[4] == 'dead'
  assert kinds[0] == 'improved' and want[4] == batch_rewards[0] > best

  dev = 'cuda'
  t = [torch.from_numpy(a.copy()).to(dev)
       for a in (pool_cont, pool_cat, rewards, perts)]
  best_t = torch.tensor([best], dtype=torch.float64, device=dev)
  iter_t = torch.zeros(12, dtype=torch.long, device=dev)
  iter_t[:2] = offset
  ext.eagle_update_f64(
      *t, torch.from_numpy(batch_cont).to(dev),
      torch.from_numpy(batch_cat).to(dev),
      torch.from_numpy(batch_rewards).to(dev),
      torch.tensor(cat_sizes, dtype=torch.long, device=dev), best_t, iter_t,
      n_batches, cfg.penalize_factor, cfg.perturbation_lower_bound,
      cfg.perturbation, seed)
  for got, expect in zip(t, want[:4]):
    assert np.array_equal(got.cpu().numpy(), expect)
  assert float(best_t[0]) == want[4]
  assert iter_t[:2].tolist() == [offset + 1, offset]
  # The refilled rows hold the widened 24-bit uniforms, over all q.
  refilled = t[0][start + 1].cpu().numpy() * 2.0 ** 24 - 0.5
  assert np.array_equal(refilled, np.round(refilled))


def test_eagle_bindings_check_their_arguments(ext):
  cfg = oracle.Config()
  inputs = _eagle_inputs(50, 4, [], seed=1)
  with pytest.raises(RuntimeError, match='pool'):
    # n_batches * batch_size beyond the pool would index past its end.
    _run_suggest(ext, *inputs, [], 5, 3, 25, 1, cfg)
  dev = 'cuda'
  with pytest.raises(RuntimeError, match='fp64'):
    ext.eagle_suggest_f64(
        torch.from_numpy(inputs[0]).float().to(dev),
        torch.from_numpy(inputs[1]).to(dev),
        torch.from_numpy(inputs[2]).to(dev),
        torch.from_numpy(inputs[3]).to(dev),
        torch.zeros(0, dtype=torch.long, device=dev),
        torch.zeros(12, dtype=torch.long, device=dev), 2, 25,
        cfg.visibility, cfg.gravity, cfg.negative_gravity,
        cfg.normalization_scale, cfg.cat_factor, cfg.p_same, 1,
        torch.empty(25, 1, 4, dtype=torch.float64, device=dev),
        torch.empty(25, 1, 0, dtype=torch.long, device=dev), 0)


# -- sweep --------------------------------------------------------------------------


def _synthetic_scoring(anchored=True):
  """ScoringFunction (UCB, trust region anchored at the training rows or
  at a copy of them) over a synthetic fp64 posterior of N = 64, D = 4 on
  the GPU."""
  from vizier_amd._src.gp import acquisitions as acq_lib
  from vizier_amd._src.gp import gp_model, matern
  g = torch.Generator().manual_seed(4)
  n, d = 64, 4
  x = torch.rand(n, d, generator=g, dtype=torch.float64)
  ls = 0.3 + 0.4 * torch.rand(d, generator=g, dtype=torch.float64)
  amp = torch.tensor(1.3, dtype=torch.float64)
  noise = torch.tensor(1e-3, dtype=torch.float64)
  mean = torch.tensor(0.25, dtype=torch.float64)
  y = torch.sin(3.0 * x.sum(-1)) - ((x - 0.6) ** 2).sum(-1)
  K = matern.gram_matern52(x, None, ls, amp) + noise * torch.eye(
      n, dtype=torch.float64)
  L = torch.linalg.cholesky(K)
  K_inv = torch.cholesky_inverse(L)
  alpha = K_inv @ (y - mean)
  params = gp_model.GPParams(amplitude=amp.cuda(), noise=noise.cuda(),
                             lengthscales=ls.cuda(), mean=mean.cuda())
  post = gp_model.GPPosterior(x=x.cuda(), params=params, L=L.cuda(),
                              alpha=alpha.cuda(), K_inv=K_inv.cuda(),
                              nll=0.0)
  trusted = post.x if anchored else post.x.clone()
  return acq_lib.ScoringFunction(post, acq_lib.UCB(coefficient=1.8),
                                 acq_lib.TrustRegion(trusted))


def _sweep(scoring, graph_safe):
  from vizier_amd._src.algorithms.optimizers import vectorized

  def score_fn(batch):
    return scoring(batch.continuous[:, 0, :])
  score_fn.graph_safe = graph_safe
  opt = vectorized.VectorizedOptimizerFactory(
      max_evaluations=1500, suggestion_batch_size=25)(
          n_continuous=4, categorical_sizes=[], seed=3, device='cuda',
          dtype=torch.float64)
  return opt, opt.optimize(score_fn, count=1)


def test_fp64_sweep_runs_captured_on_the_kernels(ext, monkeypatch):
  monkeypatch.setenv('VIZIER_AMD_FP64_HIP', '1')
  scoring = _synthetic_scoring()
  assert scoring._tr_anchored
  xs = torch.rand(25, 4, dtype=torch.float64, device='cuda')
  assert scoring._can_fuse(xs)
  opt, graphed = _sweep(scoring, graph_safe=True)
  assert opt.strategy._ext is not None and opt.strategy._f64_hip
  assert opt.last_used_graph and not opt.last_used_megakernel
  assert opt.last_graph_error is None
  assert graphed.rewards.dtype == torch.float64
  opt2, eager = _sweep(scoring, graph_safe=False)
  assert not opt2.last_used_graph and not opt2.last_used_megakernel
  assert torch.isfinite(graphed.rewards).all()
  assert torch.equal(graphed.rewards, eager.rewards)
  # The best candidate scores what the sweep recorded for it.
  again = scoring(graphed.features.continuous[:, 0, :])
  assert torch.equal(again, graphed.rewards)


def test_unanchored_trust_region_composes_on_the_f64_gram(ext, monkeypatch):
  monkeypatch.setenv('VIZIER_AMD_FP64_HIP', '1')
  scoring = _synthetic_scoring(anchored=False)
  assert not scoring._tr_anchored

  def fused(*args, **kwargs):
    raise AssertionError('the fused scorer needs an anchored trust region')
  monkeypatch.setattr(ext, 'posterior_scores_f64', fused)
  post = scoring.posterior
  xs = torch.rand(25, 4, dtype=torch.float64, device='cuda',
                  generator=torch.Generator('cuda').manual_seed(1))
  assert scoring._can_fuse(xs)
  got = scoring(xs)
  # The same composition by hand, from the fp64 HIP Gram.
  k = ext.gram_matern52_f64(xs, post.x, post.params.lengthscales, 1.3)
  quad = (k * (k @ post.K_inv)).sum(-1)
  sd = (1.3 * 1.3 - quad).clamp_min(1e-12).sqrt()
  want = 0.25 + k @ post.alpha + 1.8 * sd
  # Two evaluations of the same n-term sums differ by at most their
  # summation order: 2 n u sum|terms|, propagated through sd as above.
  n = post.x.shape[0]
  t_quad = 2.0 * n * U * ((k.abs() @ post.K_inv.abs()) * k.abs()).sum(-1)
  t_mean = 2.0 * n * U * (k.abs() @ post.alpha.abs())
  tol = t_mean + 1.8 * t_quad / (2.0 * sd)
  assert bool(((got - want).abs() <= tol).all())


def test_fp64_sweep_flag_unset_is_the_parent_path(monkeypatch):
  monkeypatch.delenv('VIZIER_AMD_FP64_HIP', raising=False)
  from vizier_amd._src.algorithms.optimizers import vectorized
  scoring = _synthetic_scoring()
  xs = torch.rand(25, 4, dtype=torch.float64, device='cuda')
  assert not scoring._can_fuse(xs)
  opt = vectorized.VectorizedOptimizerFactory(
      max_evaluations=1500, suggestion_batch_size=25)(
          n_continuous=4, categorical_sizes=[], seed=3, device='cuda',
          dtype=torch.float64)
  assert opt.strategy._ext is None
