"""GPU tests: HIP kernels vs the fp32 torch reference (run via gpurun)."""

import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def posterior_training_data(n=200, d=10, seed=0):
  """Training set of TestPosteriorScoreKernel (seeded, CPU)."""
  g = torch.Generator().manual_seed(seed)
  x = torch.rand(n, d, generator=g)
  # Real observation noise keeps the fitted noise (and cond(K)) in a
  # regime where the fp32 K_inv quadform is accurate, so the kernel
  # numerics test can be TIGHT. The near-noiseless/degenerate regime
  # is exercised end-to-end by the designer + regret evidence.
  y = torch.sin(3 * x[:, 0]) + x[:, 1] + 0.1 * torch.randn(n, generator=g)
  return x, y


@pytest.fixture(scope='module')
def ext():
  from vizier_amd._src.ops import dispatch
  e = dispatch.require_ext()  # Fails loudly if the .so is missing.
  return e


class TestGramKernel:
  """Early smoke checks; tests/test_gram_kernels.py holds these kernels to fp64."""

  @pytest.mark.parametrize('n,m,d', [(16, 16, 4), (100, 37, 20),
                                     (1000, 1000, 20), (257, 513, 51)])
  def test_cross_gram_matches_torch(self, ext, n, m, d):
    from vizier_amd._src.gp.matern import gram_matern52
    g = torch.Generator().manual_seed(0)
    x1 = torch.rand(n, d, generator=g).cuda()
    x2 = torch.rand(m, d, generator=g).cuda()
    ls = (torch.rand(d, generator=g) * 2 + 0.1).cuda()
    amp = 1.3
    got = ext.gram_matern52(x1, x2, ls, amp)
    want = gram_matern52(x1.cpu().double(), x2.cpu().double(),
                         ls.cpu().double(), torch.tensor(amp).double())
    err = (got.cpu().double() - want).abs().max()
    assert float(err) < 1e-4, f'max err {err}'

  @pytest.mark.parametrize('r,n,d', [(3, 100, 5), (12, 257, 20)])
  def test_batched_gram_matches_torch(self, ext, r, n, d):
    from vizier_amd._src.gp.matern import gram_matern52
    import math as _math
    g = torch.Generator().manual_seed(4)
    x = torch.rand(n, d, generator=g).cuda()
    ls = (torch.rand(r, d, generator=g) * 2 + 0.1).cuda()
    amp = (torch.rand(r, generator=g) + 0.5).cuda()
    noise = (torch.rand(r, generator=g) * 0.1).cuda()
    K, G = ext.gram_matern52_batched(x, ls, amp, noise, True)
    x64, ls64, amp64 = x.cpu().double(), ls.cpu().double(), \
        amp.cpu().double()
    want_k = gram_matern52(x64.unsqueeze(0), None, ls64, amp64)
    want_k = want_k + noise.cpu().double().reshape(-1, 1, 1) * \
        torch.eye(n, dtype=torch.float64)
    assert float((K.cpu().double() - want_k).abs().max()) < 1e-4
    # G = amp^2 (5/3)(1+sr) e^{-sr} with sr = sqrt5 * scaled dist.
    z = x64.unsqueeze(0) / ls64.unsqueeze(1)
    d2 = torch.cdist(z, z).pow(2).clamp_min(0)
    sr = _math.sqrt(5.0) * d2.sqrt()
    want_g = (amp64 ** 2).reshape(-1, 1, 1) * (5.0 / 3.0) * \
        (1.0 + sr) * torch.exp(-sr)
    assert float((G.cpu().double() - want_g).abs().max()) < 1e-4

  def test_fused_nll_grad_matches_torch_path(self, ext):
    """nll_value_and_grad with the fused batched gram (GPU default)
    vs the torch-composed chain (forced via CPU) at fp32 tolerance."""
    from vizier_amd._src.gp import gp_model
    g = torch.Generator().manual_seed(6)
    x = torch.rand(200, 6, generator=g)
    y = torch.sin(x[:, 0] * 3)
    raw = torch.randn(5, 9, generator=g) * 0.5
    nll_c, grad_c = gp_model.nll_value_and_grad(raw, x, y)
    nll_g, grad_g = gp_model.nll_value_and_grad(
        raw.cuda(), x.cuda(), y.cuda())
    keep = torch.isfinite(nll_c)
    assert torch.allclose(nll_g.cpu()[keep], nll_c[keep], rtol=1e-3,
                          atol=1e-2)
    scale = grad_c.abs().max()
    assert float((grad_g.cpu()[keep] - grad_c[keep]).abs().max()) < \
        max(1e-3 * float(scale), 1e-3)

  def test_symmetric_gram(self, ext):
    g = torch.Generator().manual_seed(1)
    x = torch.rand(333, 12, generator=g).cuda()
    ls = torch.full((12,), 0.7).cuda()
    K = ext.gram_matern52(x, x, ls, 2.0)
    assert torch.allclose(K, K.T, atol=1e-5)
    assert torch.allclose(torch.diagonal(K),
                          torch.full((333,), 4.0).cuda(), atol=1e-4)


class TestPosteriorScoreKernel:

  def _posterior(self):
    # The hyperparameters are one stored train_gp(num_restarts=2,
    # max_iters=20, seed=0) fit of this data: the fp32 L-BFGS fit lands
    # in a different local optimum depending on the CPU's thread count
    # and reduction order (amplitude 0.40 .. 0.54 seen), and the
    # tolerances below are statements about the kernels at ONE
    # posterior, not about the fit. The fp64 posterior cache is rebuilt
    # from them here.
    from vizier_amd._src.gp import gp_model
    x, y = posterior_training_data()
    with open(os.path.join(_GOLDEN, 'gp_posterior_n200_d10.json')) as f:
      fit = json.load(f)
    raw = torch.tensor(fit['raw'], dtype=torch.float32)
    return gp_model._build_posterior_cache(
        x, y, raw, fit['nll'], precompute_inverse=True)

  def _to_cuda(self, post):
    from vizier_amd._src.gp.gp_model import GPParams, GPPosterior
    params = GPParams(amplitude=post.params.amplitude.cuda(),
                      noise=post.params.noise.cuda(),
                      lengthscales=post.params.lengthscales.cuda(),
                      mean=post.params.mean.cuda())
    return GPPosterior(x=post.x.cuda(), params=params, L=post.L.cuda(),
                       alpha=post.alpha.cuda(),
                       K_inv=post.K_inv.cuda(), nll=post.nll,
                       noise_eff=post.noise_eff)

  def _oracle_mean_std(self, post, xq):
    """float64 posterior oracle with the cache's exact noise floor.
    The fp32 K_inv quadform (kernel AND torch fast path) carries a
    documented cancellation error ~6e-5*amp^2 in variance near the
    floor (see train_gp), so fp32-vs-fp32 comparisons are circular —
    compare both against this instead."""
    from vizier_amd._src.gp.matern import gram_matern52
    x = post.x.double()
    ls = post.params.lengthscales.double()
    amp = post.params.amplitude.double()
    K = gram_matern52(x, None, ls, amp)
    K = K + post.noise_eff * torch.eye(x.shape[0], dtype=torch.float64)
    k = gram_matern52(xq.double(), x, ls, amp)
    sol = torch.linalg.solve(K, k.T)
    mean = post.params.mean.double() + k @ post.alpha.double()
    var = (amp * amp - (k * sol.T).sum(-1)).clamp_min(1e-12)
    return mean.float(), var.sqrt().float()

  @pytest.mark.parametrize('acq,code', [('ucb', 0), ('lcb', 1), ('ei', 2),
                                        ('pi', 3)])
  def test_fused_scores_match_torch(self, ext, acq, code):
    post = self._posterior()
    gpost = self._to_cuda(post)
    g = torch.Generator().manual_seed(2)
    xq = torch.rand(64, 10, generator=g)
    mean, stddev = self._oracle_mean_std(post, xq)
    if acq == 'ucb':
      want = mean + 1.8 * stddev
    elif acq == 'lcb':
      want = mean - 1.8 * stddev
    else:
      z = (mean - 0.5) / stddev
      normal = torch.distributions.Normal(0.0, 1.0)
      if acq == 'ei':
        want = stddev * (z * normal.cdf(z) + normal.log_prob(z).exp())
      else:
        want = normal.cdf(z)
    onehot = torch.zeros(10, dtype=torch.uint8).cuda()
    got = ext.posterior_scores(
        xq.cuda(), gpost.x, gpost.params.lengthscales,
        float(gpost.params.amplitude), float(gpost.params.mean),
        gpost.alpha, gpost.K_inv, onehot, code, 1.8, 0.5, 0.0)
    # fp32 K_inv quadform error accumulates to ~1e-3*amp^2 in variance
    # (terms ~amp^2/noise_floor); at the stddev floor (~0.03*amp) that
    # is ~0.015*amp of stddev. PI/EI divide by sd, so compare them only
    # where the posterior is non-degenerate.
    amp = float(post.params.amplitude)
    got = got.cpu()
    if acq in ('pi', 'ei'):
      keep = stddev > 0.05 * amp
      assert int(keep.sum()) > 10, 'test needs non-degenerate points'
      got, want = got[keep], want[keep]
      tol = 0.02 if acq == 'pi' else 0.01 * amp
    else:
      tol = 0.01 * amp
    err = (got - want).abs().max()
    assert float(err) < tol, f'{acq}: max err {err}'

  def test_trust_region_penalty_matches(self, ext):
    from vizier_amd._src.gp import acquisitions as acq_lib
    post = self._posterior()
    gpost = self._to_cuda(post)
    tr = acq_lib.TrustRegion(post.x)
    # Points far outside the trusted region get the -1e4 - dist penalty.
    xq = torch.full((8, 10), 3.0)
    mean, stddev = post.predict(xq)
    want = tr.apply(xq, mean + 1.8 * stddev)
    onehot = torch.zeros(10, dtype=torch.uint8).cuda()
    got = ext.posterior_scores(
        xq.cuda(), gpost.x, gpost.params.lengthscales,
        float(gpost.params.amplitude), float(gpost.params.mean),
        gpost.alpha, gpost.K_inv, onehot, 0, 1.8, 0.0,
        float(tr.trust_radius))
    assert torch.allclose(got.cpu(), want, atol=1e-2)

  def test_scoring_function_uses_fused_path(self, ext):
    from vizier_amd._src.gp import acquisitions as acq_lib
    post = self._posterior()
    gpost = self._to_cuda(post)
    scoring = acq_lib.ScoringFunction(gpost, acq_lib.UCB(1.8))
    xq = torch.rand(32, 10).cuda()
    assert scoring._can_fuse(xq)
    got = scoring(xq)
    mean, stddev = self._oracle_mean_std(post, xq.cpu())
    amp = float(post.params.amplitude)
    assert torch.allclose(got.cpu(), mean + 1.8 * stddev,
                          atol=0.01 * amp)

  def test_bf16_cached_scorer_matches_fp32(self, ext):
    # The cached-operand bf16 fused scorer (posterior_scores_bf16) must
    # agree with the fp32 fused scorer to bf16-rounding tolerance, and
    # ScoringFunction(gram_dtype='bf16') must take the fused path
    # (graph-capturable; config-2 parity).
    from vizier_amd._src.gp import acquisitions as acq_lib
    post = self._posterior()
    gpost = self._to_cuda(post)
    g = torch.Generator().manual_seed(5)
    xq = torch.rand(64, 10, generator=g).cuda()
    s32 = acq_lib.ScoringFunction(gpost, acq_lib.UCB(1.8))
    s16 = acq_lib.ScoringFunction(gpost, acq_lib.UCB(1.8),
                                  gram_dtype='bf16')
    assert s16._bf16_cache is not None
    got32 = s32(xq)
    got16 = s16(xq)
    amp = float(gpost.params.amplitude)
    # bf16 rounds z = x/ls to 8 mantissa bits; the d^2 error passes
    # through the kernel and is AMPLIFIED by the variance cancellation
    # amp^2 - k^T K_inv k near training points, so score deviations
    # reach ~10% of amp at this shape (0.038 on amp 0.40 at the stored
    # fit, from a CPU emulation of the same rounding).
    # The tight rounding-exactness check against the torch bf16 oracle
    # is the next test; here we bound the drift vs full fp32.
    assert torch.allclose(got16, got32, atol=0.12 * amp)

  def test_bf16_cached_scorer_matches_torch_oracle(self, ext):
    # posterior_scores_bf16 vs a pure-torch recomputation of the SAME
    # bf16-rounded norm-trick distances (tight tolerance: identical
    # rounding, only summation order differs).
    from vizier_amd._src.gp import acquisitions as acq_lib
    post = self._posterior()
    gpost = self._to_cuda(post)
    g = torch.Generator().manual_seed(6)
    xq = torch.rand(16, 10, generator=g).cuda()
    s16 = acq_lib.ScoringFunction(gpost, acq_lib.UCB(1.8),
                                  gram_dtype='bf16')
    z2b, n2 = s16._bf16_cache
    args = (xq, gpost.x, z2b, n2, gpost.params.lengthscales,
            float(gpost.params.amplitude), float(gpost.params.mean),
            gpost.alpha, gpost.K_inv,
            torch.zeros(10, dtype=torch.uint8).cuda(), 0, 1.8, 0.0, 0.0)
    t = ext.posterior_scores_bf16(*args)
    # Torch reference of the same bf16-rounded quadform:
    z1 = (xq / gpost.params.lengthscales)
    d = z1.shape[1]
    z1b = torch.zeros(xq.shape[0], z2b.shape[1], dtype=torch.bfloat16,
                      device=xq.device)
    z1b[:, :d] = z1.to(torch.bfloat16)
    n1 = (z1b.float() ** 2).sum(-1)
    dot = z1b.float() @ z2b.float().T
    d2 = (n1[:, None] + n2[None, :] - 2 * dot).clamp_min(0)
    r = d2.sqrt()
    sr = (5.0 ** 0.5) * r
    amp = float(gpost.params.amplitude)
    kv = amp * amp * (1 + sr + sr * sr / 3) * torch.exp(-sr)
    mu = float(gpost.params.mean) + kv @ gpost.alpha
    var = (amp * amp -
           (kv * (kv @ gpost.K_inv)).sum(-1)).clamp_min(1e-12)
    want = mu + 1.8 * var.sqrt()
    assert torch.allclose(t, want, atol=0.02 * amp)


class TestUCBPEFusedPaths:

  def _designer(self, n_trials=30):
    from vizier_amd import pyvizier as vz
    from vizier_amd._src.algorithms.core.abstractions import (
        ActiveTrials,
        CompletedTrials,
    )
    from vizier_amd._src.algorithms.designers.gp_ucb_pe import (
        UCBPEConfig,
        VizierGPUCBPEBandit,
    )
    problem = vz.ProblemStatement()
    for i in range(5):
      problem.search_space.root.add_float_param(f'x{i}', 0.0, 1.0)
    problem.metric_information.append(vz.MetricInformation(
        name='obj', goal=vz.ObjectiveMetricGoal.MAXIMIZE))
    d = VizierGPUCBPEBandit(problem, UCBPEConfig(
        max_evaluations=500, ard_restarts=1, ard_max_iters=10,
        device='cuda'), seed=0)
    rng = np.random.default_rng(0)
    trials = []
    for uid in range(1, n_trials + 1):
      x = rng.uniform(0, 1, 5)
      t = vz.Trial({f'x{i}': float(x[i]) for i in range(5)}, id=uid)
      t.complete(vz.Measurement(
          metrics={'obj': float(-((x - 0.6) ** 2).sum())}))
      trials.append(t)
    d.update(CompletedTrials(trials), ActiveTrials())
    d._fit()
    return d

  def test_fused_pe_matches_eager(self, ext):
    """The fused PE scorer (two posterior_mean_std kernel calls) must
    reproduce the eager predict chain."""
    import vizier_amd._src.gp.acquisitions as acq_lib
    from vizier_amd._src.algorithms.optimizers.eagle import (
        CandidateBatch,
    )
    d = self._designer()
    cfg = d._config
    posterior = d._posterior
    x_all = posterior.x
    tr = acq_lib.TrustRegion.for_converter(x_all, d._converter)
    var_post = d._variance_posterior(x_all)
    assert d._fusable(posterior) and d._fusable(var_post, x_all)

    g = torch.Generator().manual_seed(4)
    xs = torch.rand(40, 1, 5, generator=g).cuda()
    batch = CandidateBatch(xs, torch.zeros(40, 1, 0, dtype=torch.long,
                                           device='cuda'))
    # Fused score_fn comes out of _optimize_one's machinery; rebuild
    # both paths directly for a clean comparison.
    import vizier_amd_hip as hip_ext
    onehot, radius = d._tr_kernel_args(tr, x_all.device)
    mean_obs, stddev_obs = posterior.predict(posterior.x)
    ucb_obs = mean_obs + cfg.ucb_coefficient * stddev_obs
    threshold = mean_obs[int(torch.argmax(ucb_obs))]
    flat = xs[:, 0, :]
    m, sdev, _ = hip_ext.posterior_mean_std(
        flat, posterior.x, posterior.params.lengthscales,
        float(posterior.params.amplitude),
        float(posterior.params.mean), posterior.alpha,
        posterior.K_inv, onehot)
    _, s_all, dist = hip_ext.posterior_mean_std(
        flat, var_post.x, var_post.params.lengthscales,
        float(var_post.params.amplitude), 0.0, var_post.alpha,
        var_post.K_inv, onehot)
    explore = m + cfg.explore_region_ucb_coefficient * sdev
    pen = cfg.cb_violation_penalty_coefficient * torch.minimum(
        explore - float(threshold), torch.zeros_like(explore))
    fused = s_all + pen
    if radius <= 0.5:
      fused = torch.where(dist <= radius, fused, -1e4 - dist)
    # Eager oracle.
    mean_e, stddev_e = posterior.predict(flat)
    explore_e = mean_e + cfg.explore_region_ucb_coefficient * stddev_e
    _, s_all_e = var_post.predict(flat)
    pen_e = cfg.cb_violation_penalty_coefficient * torch.minimum(
        explore_e - threshold, torch.zeros_like(explore_e))
    want = tr.apply(flat, s_all_e + pen_e)
    amp = float(posterior.params.amplitude)
    assert torch.allclose(fused, want, atol=0.02 * amp),         float((fused - want).abs().max())


class TestBatchedCholesky:

  def test_potrf_matches_torch(self, ext):
    g = torch.Generator().manual_seed(11)
    for n in (33, 200, 1000):
      A = torch.randn(6, n, 48, generator=g)
      K = (A @ A.mT / 48 + torch.eye(n)).cuda().contiguous()
      L, info = ext.batched_potrf(K)
      want = torch.linalg.cholesky(K)
      assert int(info.abs().sum()) == 0
      err = (torch.tril(L) - want).abs().max()
      assert float(err) < 5e-4, f'n={n}: {err}'

  def test_potrf_flags_non_pd(self, ext):
    K = torch.eye(64).repeat(3, 1, 1).cuda().contiguous()
    K[1, 10, 10] = -1.0
    _, info = ext.batched_potrf(K)
    assert int(info[0]) == 0 and int(info[2]) == 0
    assert int(info[1]) == 11  # 1-based failing column

  def test_potrf_edge_shapes(self, ext):
    """Edge shapes: single matrix, odd N, batch 12 (the line-search
    ladder), and N crossing many panel rounds."""
    g = torch.Generator().manual_seed(17)
    for r, n in ((1, 257), (3, 999), (12, 1000), (2, 64), (4, 65)):
      A = torch.randn(r, n, 32, generator=g)
      K = (A @ A.mT / 32 + torch.eye(n)).cuda().contiguous()
      L, info = ext.batched_potrf(K)
      want = torch.linalg.cholesky(K)
      assert int(info.abs().sum()) == 0, f'r={r} n={n}'
      err = (torch.tril(L) - want).abs().max()
      assert float(err) < 5e-4, f'r={r} n={n}: {err}'

  def test_potrf_flags_non_pd_across_panels(self, ext):
    # Failure column inside a later panel round.
    K = torch.eye(300).repeat(2, 1, 1).cuda().contiguous()
    K[0, 170, 170] = -2.0
    _, info = ext.batched_potrf(K)
    assert int(info[1]) == 0
    assert int(info[0]) == 171

  def test_trsv_matches_torch(self, ext):
    g = torch.Generator().manual_seed(12)
    for n in (50, 1000):
      A = torch.randn(5, n, 32, generator=g)
      K = (A @ A.mT / 32 + torch.eye(n)).cuda()
      L = torch.linalg.cholesky(K).contiguous()
      b = torch.randn(5, n, generator=g).cuda().contiguous()
      got = ext.batched_trsv_lower(L, b)
      want = torch.linalg.solve_triangular(
          L, b.unsqueeze(-1), upper=False).squeeze(-1)
      err = (got - want).abs().max()
      assert float(err) < 5e-4, f'n={n}: {err}'

  def test_nll_custom_path_matches_torch(self, ext, monkeypatch):
    monkeypatch.setenv('VIZIER_AMD_CUSTOM_CHOL', '1')
    from vizier_amd._src.gp import gp_model
    g = torch.Generator().manual_seed(13)
    x = torch.rand(300, 6, generator=g).cuda()
    y = torch.sin(x[:, 0] * 3).cuda()
    raw = torch.randn(8, 9, generator=g).cuda()
    with torch.no_grad():
      got = gp_model.negative_log_marginal_likelihood(raw, x, y)
    # Force the torch path by requiring grad on raw.
    raw2 = raw.clone().requires_grad_(True)
    want = gp_model.negative_log_marginal_likelihood(raw2, x, y)
    keep = torch.isfinite(want)
    assert torch.allclose(got[keep], want.detach()[keep], rtol=1e-3,
                          atol=1e-2)


class TestEagleKernels:

  def test_suggest_statistics_match_torch_path(self, ext):
    """HIP suggest: same force/move math (RNG streams differ), so with
    zero perturbation the continuous move must match exactly."""
    from vizier_amd._src.algorithms.optimizers import eagle as eagle_lib

    def build(device):
      s = eagle_lib.VectorizedEagleStrategy(
          n_continuous=6, categorical_sizes=[3], batch_size=5,
          seed=3, device=device)
      return s

    cpu = build('cpu')
    state_c = cpu.init_state()
    # Fill rewards so we're in steady state, mirrored on GPU.
    n_init = cpu.pool_size // cpu.batch_size
    g = torch.Generator().manual_seed(0)
    rewards = torch.rand(cpu.pool_size, generator=g)
    state_c.rewards = rewards.clone()
    state_c.iterations = n_init
    state_c.perturbations.zero_()  # suppress noise for determinism

    gpu = build('cuda')
    state_g = gpu.init_state()
    state_g.continuous = state_c.continuous.cuda()
    state_g.categorical = state_c.categorical.cuda()
    state_g.rewards = rewards.cuda()
    state_g.perturbations.zero_()
    state_g.iterations = n_init

    out_c = cpu.suggest(state_c)
    out_g = gpu.suggest(state_g)
    err = (out_c.continuous - out_g.continuous.cpu()).abs().max()
    assert float(err) < 1e-4, f'move mismatch {err}'
    # The categories are the NumPy oracle's (tests/eagle_f64_oracle.py:
    # the kernel's RNG bit for bit, formulas in float64), wherever its
    # top-2 `logit + gumbel` margin exceeds tau = 4 x the
    # float32-vs-float64 difference of that sum; every entry does.
    import eagle_f64_oracle as oracle
    assert out_g.categorical.shape == out_c.categorical.shape
    c = gpu.config
    args = (state_c.continuous.numpy(), state_c.categorical.numpy(),
            rewards.numpy(), np.zeros(cpu.pool_size, dtype=np.float32), [3],
            n_init, n_init, cpu.batch_size, 3,
            oracle.Config(
                visibility=c.visibility, gravity=c.gravity,
                negative_gravity=c.negative_gravity,
                normalization_scale=c.normalization_scale,
                cat_factor=c.categorical_perturbation_factor,
                p_same=c.prob_same_category_without_perturbation))
    _, want_cat, margin, vals64 = oracle.suggest(
        *args, dtype=np.float32, arith=np.float64, return_vals=True)
    vals32 = oracle.suggest(*args, dtype=np.float32, arith=np.float32,
                            return_vals=True)[3]
    tau = 4.0 * float(np.nanmax(np.abs(vals32 - vals64)))
    assert margin > tau, (margin, tau)
    assert np.array_equal(out_g.categorical.cpu().numpy(), want_cat)

  def test_update_accept_reject(self, ext):
    from vizier_amd._src.algorithms.optimizers import eagle as eagle_lib
    s = eagle_lib.VectorizedEagleStrategy(
        n_continuous=4, categorical_sizes=[], batch_size=5, seed=0,
        device='cuda')
    state = s.init_state()
    n_init = s.pool_size // s.batch_size
    # Drive through init phase.
    for _ in range(n_init):
      batch = s.suggest(state)
      r = -((batch.continuous[:, 0, :] - 0.5) ** 2).sum(-1)
      state = s.update(state, batch, r)
    assert torch.isfinite(state.rewards).all()
    r_before = state.rewards.clone()
    batch = s.suggest(state)
    worse = torch.full((5,), -100.0).cuda()
    state = s.update(state, batch, worse)
    sl = slice(0, 5)
    # Rejected: rewards unchanged, perturbations decayed.
    assert torch.allclose(state.rewards[sl], r_before[sl])
    assert (state.perturbations[sl] < 0.16).all()


class TestEagleSweepMegakernel:

  def _make_problem(self, n=300, d=12, seed=0):
    from vizier_amd._src.gp import acquisitions as acq_lib
    from vizier_amd._src.gp import gp_model
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, d, generator=g).cuda()
    y = (-((x - 0.4) ** 2).sum(-1) +
         0.01 * torch.randn(n, generator=g).cuda())
    post = gp_model.train_gp(x, y, num_restarts=2, max_iters=15)
    onehot = torch.zeros(d, dtype=torch.bool, device='cuda')
    tr = acq_lib.TrustRegion(post.x, onehot)
    scoring = acq_lib.ScoringFunction(
        post, acq_lib.UCB(coefficient=1.8), tr)
    return post, scoring, d

  def _run(self, scoring, d, *, force_graph, evals=5000, seed=7):
    import os
    os.environ['VIZIER_AMD_MEGAKERNEL'] = '1'
    from vizier_amd._src.algorithms.optimizers.eagle import (
        EagleStrategyConfig)
    from vizier_amd._src.algorithms.optimizers.vectorized import (
        VectorizedOptimizerFactory)
    factory = VectorizedOptimizerFactory(
        eagle_config=EagleStrategyConfig(), max_evaluations=evals,
        suggestion_batch_size=25)
    opt = factory(n_continuous=d, categorical_sizes=[], n_parallel=1,
                  seed=seed, device='cuda', dtype=torch.float32)
    if force_graph:
      opt._megakernel_applicable = lambda score_fn: False

    def score_fn(batch):
      return scoring(batch.continuous[:, 0, :])
    score_fn.scoring = scoring
    score_fn.codec_identity = True
    res = opt.optimize(score_fn, count=3)
    return opt, res

  def test_megakernel_bitwise_matches_hipgraph(self, ext):
    """The persistent cooperative sweep must produce EXACTLY the same
    pool trajectory as the hipGraph path (same RNG streams, same
    NCHUNK partition, same reduce orders)."""
    post, scoring, d = self._make_problem()
    opt_g, res_g = self._run(scoring, d, force_graph=True)
    assert opt_g.last_used_graph, opt_g.last_graph_error
    opt_m, res_m = self._run(scoring, d, force_graph=False)
    assert opt_m.last_used_megakernel, opt_m.last_graph_error
    assert torch.equal(res_m.rewards, res_g.rewards)
    assert torch.equal(res_m.features.continuous,
                       res_g.features.continuous)

  def test_megakernel_finds_optimum_region(self, ext):
    post, scoring, d = self._make_problem()
    opt, res = self._run(scoring, d, force_graph=False, evals=10000)
    assert opt.last_used_megakernel
    best = res.features.continuous[0, 0, :]
    # UCB over a GP fit to -(x-0.4)^2 peaks near 0.4.
    assert float((best - 0.4).abs().mean()) < 0.2


class TestGPUDesignerEndToEnd:

  def test_gp_bandit_on_gpu(self, ext):
    from vizier_amd import pyvizier as vz
    from vizier_amd._src.algorithms.core.abstractions import (
        ActiveTrials,
        CompletedTrials,
    )
    from vizier_amd._src.algorithms.designers.gp_bandit import (
        GPBanditConfig,
        VizierGPBandit,
    )
    problem = vz.ProblemStatement()
    for i in range(8):
      problem.search_space.root.add_float_param(f'x{i}', 0.0, 1.0)
    problem.metric_information.append(vz.MetricInformation(
        name='obj', goal=vz.ObjectiveMetricGoal.MAXIMIZE))
    designer = VizierGPBandit(problem, GPBanditConfig(
        max_evaluations=2000, ard_restarts=2, ard_max_iters=20,
        device='cuda'), seed=0)
    uid = 0
    best = -np.inf
    for _ in range(12):
      for s in designer.suggest(1):
        uid += 1
        x = np.array([s.parameters.get_value(f'x{i}') for i in range(8)])
        val = float(-((x - 0.3) ** 2).sum())
        best = max(best, val)
        t = s.to_trial(uid)
        t.complete(vz.Measurement(metrics={'obj': val}))
        designer.update(CompletedTrials([t]), ActiveTrials())
    assert best > -0.25, f'GPU GP-Bandit failed to converge: {best}'

  def test_gp_bandit_fp64_mode_on_gpu(self, ext):
    # The --fp64 parity mode (reference forces jax x64): HIP fp32
    # kernels are bypassed, the whole pipeline runs float64 on rocBLAS
    # DGEMMs, and suggestions are still sane.
    from vizier_amd import pyvizier as vz
    from vizier_amd._src.algorithms.core.abstractions import (
        ActiveTrials,
        CompletedTrials,
    )
    from vizier_amd._src.algorithms.designers.gp_bandit import (
        GPBanditConfig,
        VizierGPBandit,
    )
    problem = vz.ProblemStatement()
    for i in range(4):
      problem.search_space.root.add_float_param(f'x{i}', 0.0, 1.0)
    problem.metric_information.append(vz.MetricInformation(
        name='obj', goal=vz.ObjectiveMetricGoal.MAXIMIZE))
    designer = VizierGPBandit(problem, GPBanditConfig(
        max_evaluations=800, ard_restarts=1, ard_max_iters=10,
        device='cuda', dtype=torch.float64), seed=0)
    uid = 0
    for _ in range(4):
      for s in designer.suggest(1):
        uid += 1
        x = np.array([s.parameters.get_value(f'x{i}')
                      for i in range(4)])
        t = s.to_trial(uid)
        t.complete(vz.Measurement(
            metrics={'obj': float(-((x - 0.4) ** 2).sum())}))
        designer.update(CompletedTrials([t]), ActiveTrials())
    assert designer._x.dtype == torch.float64
    mean, _ = designer._posteriors[0].predict(designer._x[:2])
    assert mean.dtype == torch.float64

  def test_fused_mo_scorer_matches_eager_chain(self, ext):
    """The fused MO path (posterior_mean_std + hv_scalarize_tr) must
    reproduce the eager python scalarization chain."""
    from vizier_amd import pyvizier as vz
    from vizier_amd._src.algorithms.core.abstractions import (
        ActiveTrials,
        CompletedTrials,
    )
    from vizier_amd._src.algorithms.designers.gp_bandit import (
        GPBanditConfig,
        VizierGPBandit,
    )
    from vizier_amd._src.algorithms.optimizers.eagle import CandidateBatch
    rng = np.random.default_rng(3)
    problem = vz.ProblemStatement()
    for i in range(4):
      problem.search_space.root.add_float_param(f'x{i}', 0.0, 1.0)
    problem.metric_information = vz.MetricsConfig([
        vz.MetricInformation(name=n, goal=vz.ObjectiveMetricGoal.MAXIMIZE)
        for n in ('f1', 'f2')])
    designer = VizierGPBandit(problem, GPBanditConfig(
        max_evaluations=500, ard_restarts=1, ard_max_iters=10,
        device='cuda'), seed=0)
    trials = []
    for uid in range(1, 13):
      x = rng.uniform(0, 1, 4)
      t = vz.Trial({f'x{i}': float(x[i]) for i in range(4)}, id=uid)
      t.complete(vz.Measurement(metrics={
          'f1': float(-((x - 0.2) ** 2).sum()),
          'f2': float(-((x - 0.8) ** 2).sum())}))
      trials.append(t)
    designer.update(CompletedTrials(trials), ActiveTrials())
    designer._fit()
    fused_fn, _ = designer._score_factory(1)
    assert getattr(fused_fn, 'graph_safe', False), \
        'fused MO path did not engage'
    # Build the eager chain by disabling the fused conditions.
    designer._config.scorer_gram_dtype = 'fp32'
    mt_save = designer._mt_posterior

    class _Blocker:
      pass
    designer._mt_posterior = None
    kinv_save = designer._posteriors[0].K_inv
    xs = torch.rand(32, 1, 4, generator=torch.Generator().manual_seed(1)
                    ).cuda()
    batch = CandidateBatch(xs, torch.zeros(32, 1, 0, dtype=torch.long,
                                           device='cuda'))
    got = fused_fn(batch)
    # Eager oracle: per-metric predict + python scalarizer + TR.
    import vizier_amd._src.gp.acquisitions as acq_lib
    tr = designer._make_trust_region()
    scal = acq_lib.create_hv_scalarization(
        designer._config.num_scalarizations, 2, seed=designer._seed,
        reference_point=acq_lib.get_reference_point(
            designer._warped_labels,
            scale=designer._config.ref_scaling))
    flat = xs[:, 0, :]
    ys = torch.stack(
        [m + 1.8 * s for m, s in
         (p.predict(flat) for p in designer._posteriors)], dim=-1)
    want = scal(ys).mean(dim=0)
    want = tr.apply(flat, want)
    designer._mt_posterior = mt_save
    assert torch.allclose(got, want, atol=2e-3), \
        float((got - want).abs().max())

  def test_multi_objective_and_qei_on_gpu(self, ext):
    """MO hypervolume-scalarized scoring and q-EI batches run the full
    GPU path (catches device-placement regressions in the composed
    scorers that the fast single-objective path doesn't exercise)."""
    from vizier_amd import pyvizier as vz
    from vizier_amd._src.algorithms.core.abstractions import (
        ActiveTrials,
        CompletedTrials,
    )
    from vizier_amd._src.algorithms.designers.gp_bandit import (
        GPBanditConfig,
        VizierGPBandit,
    )
    rng = np.random.default_rng(0)

    # Multi-objective: two conflicting objectives.
    problem = vz.ProblemStatement()
    for i in range(4):
      problem.search_space.root.add_float_param(f'x{i}', 0.0, 1.0)
    problem.metric_information = vz.MetricsConfig([
        vz.MetricInformation(name=n, goal=vz.ObjectiveMetricGoal.MAXIMIZE)
        for n in ('f1', 'f2')])
    designer = VizierGPBandit(problem, GPBanditConfig(
        max_evaluations=1500, ard_restarts=1, ard_max_iters=10,
        device='cuda'), seed=0)
    uid = 0
    for _ in range(6):
      for s in designer.suggest(1):
        uid += 1
        x = np.array([s.parameters.get_value(f'x{i}') for i in range(4)])
        t = s.to_trial(uid)
        t.complete(vz.Measurement(metrics={
            'f1': float(-((x - 0.2) ** 2).sum()),
            'f2': float(-((x - 0.8) ** 2).sum())}))
        designer.update(CompletedTrials([t]), ActiveTrials())

    # q-EI: batches of 3 distinct suggestions.
    problem2 = vz.ProblemStatement()
    for i in range(4):
      problem2.search_space.root.add_float_param(f'x{i}', 0.0, 1.0)
    problem2.metric_information.append(vz.MetricInformation(
        name='obj', goal=vz.ObjectiveMetricGoal.MAXIMIZE))
    d2 = VizierGPBandit(problem2, GPBanditConfig(
        max_evaluations=1500, acquisition='qei', ard_restarts=1,
        ard_max_iters=10, device='cuda'), seed=1)
    uid = 0
    for _ in range(4):
      batch = d2.suggest(3)
      assert len(batch) == 3
      rows = [tuple(round(s.parameters.get_value(f'x{i}'), 6)
                    for i in range(4)) for s in batch]
      trials = []
      for s in batch:
        uid += 1
        x = np.array([s.parameters.get_value(f'x{i}') for i in range(4)])
        t = s.to_trial(uid)
        t.complete(vz.Measurement(
            metrics={'obj': float(-((x - 0.5) ** 2).sum())}))
        trials.append(t)
      d2.update(CompletedTrials(trials), ActiveTrials())
    assert len(set(rows)) > 1, 'qEI produced identical batch points'


class TestGramBf16MFMA:
  """Early smoke checks; tests/test_gram_kernels.py holds these kernels to fp64."""

  @pytest.mark.parametrize('n,m,d', [(64, 64, 20), (500, 500, 8),
                                     (257, 130, 51)])
  def test_bf16_mfma_matches_fp64_reference(self, ext, n, m, d):
    from vizier_amd._src.gp.matern import gram_matern52
    g = torch.Generator().manual_seed(7)
    x1 = torch.rand(n, d, generator=g).cuda()
    x2 = torch.rand(m, d, generator=g).cuda()
    ls = (torch.rand(d, generator=g) * 1.5 + 0.2).cuda()
    amp = 1.4
    got = ext.gram_matern52_bf16(x1, x2, ls, amp)
    want = gram_matern52(x1.cpu().double(), x2.cpu().double(),
                         ls.cpu().double(), torch.tensor(amp).double())
    err = (got.cpu().double() - want).abs().max()
    # bf16 cross-term: ~3 decimal digits; kernel values are O(amp^2).
    assert float(err) < 3e-2 * amp * amp, f'max err {err}'
    # Asymmetric inputs catch operand/output transposes (guide G9): the
    # error against the TRANSPOSED reference must be much larger.
    err_t = (got.cpu().double() - want.T).abs().max() if n == m else None
    if err_t is not None:
      assert float(err_t) > 10 * float(err)

  @pytest.mark.parametrize('n,m,d', [(128, 130, 32), (640, 520, 20),
                                     (1111, 777, 90)])
  def test_bf16_lds_tiled_matches_fp64_reference(self, ext, n, m, d):
    """The 128x128 LDS-tiled MFMA path (incl. ragged tile edges)."""
    from vizier_amd._src.gp.matern import gram_matern52
    g = torch.Generator().manual_seed(3)
    x1 = torch.rand(n, d, generator=g).cuda()
    x2 = torch.rand(m, d, generator=g).cuda()
    ls = (torch.rand(d, generator=g) * 1.5 + 0.2).cuda()
    amp = 1.3
    got = ext.gram_matern52_bf16_tiled(x1, x2, ls, amp)
    want = gram_matern52(x1.cpu().double(), x2.cpu().double(),
                         ls.cpu().double(), torch.tensor(amp).double())
    err = (got.cpu().double() - want).abs().max()
    assert float(err) < 3e-2 * amp * amp, f'max err {err}'

  def test_bf16_diag_is_amp2(self, ext):
    x = torch.rand(100, 16).cuda()
    ls = torch.full((16,), 0.5).cuda()
    K = ext.gram_matern52_bf16(x, x, ls, 2.0)
    assert torch.allclose(torch.diagonal(K),
                          torch.full((100,), 4.0).cuda(), atol=0.05)


class TestGramFp8MFMA:
  """Early smoke checks; tests/test_gram_kernels.py holds these kernels to fp64."""

  @pytest.mark.parametrize('n,m,d', [(128, 130, 32), (1111, 777, 90)])
  def test_fp8_lds_tiled_matches_fp64_loosely(self, ext, n, m, d):
    from vizier_amd._src.gp.matern import gram_matern52
    g = torch.Generator().manual_seed(13)
    x1 = torch.rand(n, d, generator=g).cuda()
    x2 = torch.rand(m, d, generator=g).cuda()
    ls = (torch.rand(d, generator=g) * 1.5 + 0.3).cuda()
    got = ext.gram_matern52_fp8_tiled(x1, x2, ls, 1.0)
    want = gram_matern52(x1.cpu().double(), x2.cpu().double(),
                         ls.cpu().double(), torch.tensor(1.0).double())
    err = (got.cpu().double() - want).abs().max()
    assert float(err) < 0.15, f'max err {err}'  # e4m3: ~2 digits

  def test_fp8_mfma_matches_fp64_loosely(self, ext):
    from vizier_amd._src.gp.matern import gram_matern52
    g = torch.Generator().manual_seed(11)
    x1 = torch.rand(128, 30, generator=g).cuda()
    x2 = torch.rand(96, 30, generator=g).cuda()
    ls = (torch.rand(30, generator=g) * 1.5 + 0.3).cuda()
    amp = 1.0
    got = ext.gram_matern52_fp8(x1, x2, ls, amp)
    want = gram_matern52(x1.cpu().double(), x2.cpu().double(),
                         ls.cpu().double(), torch.tensor(amp).double())
    err = (got.cpu().double() - want).abs().max()
    # e4m3 has ~2 significant digits; the Gram is O(1).
    assert float(err) < 0.15, f'max err {err}'

  def test_fp8_cached_gram_matches_per_call(self, ext):
    # Fp8GramCache (operand cache, deterministic unit-box scale, no
    # per-call host sync) vs the per-call conversion path vs fp32 —
    # all three agree to e4m3 tolerance.
    from vizier_amd._src.gp import acquisitions as acq_lib
    g = torch.Generator().manual_seed(9)
    x = torch.rand(200, 12, generator=g).cuda()
    xq = torch.rand(25, 12, generator=g).cuda()
    ls = (torch.rand(12, generator=g) * 0.8 + 0.4).cuda()
    cache = acq_lib.Fp8GramCache(x, ls, amplitude=1.3)
    got = cache.gram(xq)
    percall = ext.gram_matern52_fp8(xq, x, ls, 1.3)
    fp32 = ext.gram_matern52(xq, x, ls, 1.3)
    assert float((got - fp32).abs().max()) < 0.15
    assert float((percall - fp32).abs().max()) < 0.15
    assert float((got - percall).abs().max()) < 0.2

  def test_fp8_fused_mean_std_matches_cached_gram(self, ext):
    # posterior_mean_std_fp8 (kernel-side e4m3fn decode) must agree
    # with the torch Fp8GramCache composed math on the same operands.
    from vizier_amd._src.gp import acquisitions as acq_lib
    from vizier_amd._src.gp import gp_model
    g = torch.Generator().manual_seed(21)
    x = torch.rand(150, 8, generator=g)
    y = torch.sin(3 * x[:, 0]) + 0.1 * torch.randn(150, generator=g)
    post = gp_model.train_gp(x, y, num_restarts=1, max_iters=15,
                             seed=3)
    from vizier_amd._src.gp.gp_model import GPParams, GPPosterior
    params = GPParams(amplitude=post.params.amplitude.cuda(),
                      noise=post.params.noise.cuda(),
                      lengthscales=post.params.lengthscales.cuda(),
                      mean=post.params.mean.cuda())
    gp = GPPosterior(x=post.x.cuda(), params=params, L=post.L.cuda(),
                     alpha=post.alpha.cuda(), K_inv=post.K_inv.cuda(),
                     nll=post.nll)
    cache = acq_lib.Fp8GramCache(gp.x, gp.params.lengthscales,
                                 float(gp.params.amplitude))
    xq = torch.rand(25, 8, generator=g).cuda()
    onehot = torch.zeros(8, dtype=torch.uint8).cuda()
    mean, sd, dist = ext.posterior_mean_std_fp8(
        xq, gp.x, cache.z2q, cache.n2, cache.scale,
        gp.params.lengthscales, float(gp.params.amplitude),
        float(gp.params.mean), gp.alpha, gp.K_inv, onehot)
    # Oracle with torch's EXACT e4m3 dequantization (the kernel's
    # software decode must match it bitwise; the MFMA gram kernel is a
    # different fp8 dot implementation and only agrees to fp8
    # tolerance).
    d = 8
    dp = cache.dp
    z1 = xq / gp.params.lengthscales
    z1q = torch.zeros(25, dp, dtype=torch.float8_e4m3fn, device='cuda')
    z1q[:, :d] = (z1 / cache.scale).to(torch.float8_e4m3fn)
    z1f = z1q.to(torch.float32) * cache.scale
    n1 = (z1f * z1f).sum(-1)
    z2f = cache.z2q.to(torch.float32) * cache.scale
    d2 = (n1[:, None] + cache.n2[None, :] - 2 * z1f @ z2f.T).clamp_min(0)
    r = d2.sqrt()
    sr = (5.0 ** 0.5) * r
    amp2 = float(gp.params.amplitude) ** 2
    k = amp2 * (1 + sr + sr * sr / 3) * torch.exp(-sr)
    want_mean = float(gp.params.mean) + k @ gp.alpha
    want_var = (amp2 - (k * (k @ gp.K_inv)).sum(-1)).clamp_min(1e-12)
    assert torch.allclose(mean, want_mean, atol=1e-3),         float((mean - want_mean).abs().max())
    assert torch.allclose(sd, want_var.sqrt(), atol=5e-3)
    # And the MFMA cached-gram path agrees to fp8-level tolerance.
    k_mfma = cache.gram(xq)
    assert float((k_mfma - k).abs().max()) < 0.2
    # Trust-region distance: min L-inf to the training rows.
    want_dist = (xq.unsqueeze(1) - gp.x).abs().amax(-1).amin(-1)
    assert torch.allclose(dist, want_dist, atol=1e-5)

  def test_fp8_diag_near_exact(self, ext):
    x = torch.rand(64, 16).cuda()
    ls = torch.full((16,), 0.5).cuda()
    K = ext.gram_matern52_fp8(x, x, ls, 2.0)
    # Norms come from the rounded values, so the diagonal is exact up
    # to fp32 summation-order differences (measured 3e-3).
    assert torch.allclose(torch.diagonal(K),
                          torch.full((64,), 4.0).cuda(), atol=1e-2)
