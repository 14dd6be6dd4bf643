"""Designers with installed posteriors, candidates on both sides of the trust
radius, and fp64 oracles of the scorers the designers hand to the sweep.

The kernels are held to fp64 oracles on synthetic operands elsewhere
(scorer_cases.py and its neighbours). What is checked HERE is the layer that
feeds them: the closures of VizierGPUCBPEBandit._one_score_fn and
VizierGPBandit._score_factory choose which posterior, which K^-1, which
threshold, which one-hot mask, which radius and which distance go into the
kernels. Shared by tests/test_designer_cases.py (CPU self-check) and
tests/test_designer_scorers.py (GPU).

Problems
  float   4 float parameters.
  mixed   x0, k (integer 0..3), x1, c (3-way categorical), x2: feature columns
          [x0, k, x1, c0, c1, c2, x2]. k's scaled gap is 1/3 > 0.2, so the
          trust region excludes column 1 and the one-hot block 3..5: the
          excluded columns are NOT contiguous. dof = 3 + 1 in both problems.
  One or two metrics.

Designers: 12 completed trials, 0 or 2 pending, ard_restarts=1,
ard_max_iters=10. After _fit() every posterior is REPLACED by
gp_model._build_posterior_cache at chosen hyperparameters (amp 1.3, noise
1e-2 amp^2, mean 0.25, distinct lengthscales in [0.3, 0.8], reversed for the
second metric): the fit is not under test, the conditioning is controlled.
The linear-kernel designer gets a LinearMaternPosterior built the same way.

Trials keep their included coordinates in [0.05, 0.5], k in {0, 1} and the
categories a, b. Candidates (B = 32): 16 within 0.05 (L-inf, included
columns) of a trusted row, most of them with excluded columns at least 0.5
from every trusted row (make_candidates); 16 with one included column in
[0.93, 1], i.e. at least radius + 0.05 from every trusted row (radius 0.344
at 12 rows, 0.368 at 14). The hypervolume scalarization uses 7 directions: a
set that small is visibly asymmetric, so swapped metrics show.

Oracle: every score from its formula in float64 on the designer's stored
operands upcast (x, lengthscales, float(amp), float(mean), alpha, K_inv or
L); fp8 / bf16 on the quantised operands via scorer_cases.reference_lowp.

Tolerances (per candidate, from the reference):
  |d var|  <= 10 (2 * 2e-6 + N eps32) (prior + sum_ij |k_i||M_ij||k_j|)
  |d mean| <= 10 (2e-6 + N eps32) sum_i |k_i||alpha_i|
  |d sd|   <= |d var| / (2 sd_ref)
2e-6 is the k-vector's relative error (__expf and the fp32 distance) and 10
the margin, both as scorer_cases.TOL_FP32; N eps32 is the fp32 summation.
Scores combine these linearly: |coef|, the penalty coefficient (whenever the
penalty is active or within its own error of it; the threshold's own |d
mean| at the observed point is included), and for the hypervolume
scalarization, per direction v, max_m |d y_m| / w_vm + 4 eps32 |s_v| over
the metrics m that can be the argmin at all (those whose lower end is not
above the smallest upper end), averaged over v, plus V eps32 mean_v |s_v|
for the fp32 mean over V values. Since |min_m a - min_m b| <= max_m |a - b|
this is never above the plain 1 / min(weight) bound. Candidates outside the
radius score -1e4 - dist and are held to scorer_cases.TOL_PENALTY. fp8 / bf16: scorer_cases.lowp_bounds.
"""

import dataclasses
import functools
import math
from typing import List, Optional

import numpy as np
import torch

import gram_cases as gc
import scorer_cases as sc

AMP = sc.AMP
NOISE = 1e-2 * AMP * AMP
MEAN_C = sc.MEAN_C
N_DONE = 12
B = 32
NEAR = 0.05
TRIAL_LO, TRIAL_HI = 0.05, 0.5
FAR_LO = 0.93
EPS32 = 2.0 ** -23
K_REL = 2e-6
MARGIN = 10.0
DOF = 4
N_DIRECTIONS = 7
LIN_SLOPE, LIN_SHIFT = 0.3, 0.2

# feature-column masks the trust region must use (1 = excluded)
MASKS = {'float': [0, 0, 0, 0], 'mixed': [0, 1, 0, 1, 1, 1, 0]}


def radius(n_rows: int) -> float:
  """TrustRegion's radius, written out: 0.2 + 0.3 n / (5 (dof + 1))."""
  return 0.2 + (0.5 - 0.2) * n_rows / (5.0 * (DOF + 1))


def lengthscales(d: int, metric: int) -> List[float]:
  ls = [0.3 + 0.5 * (i / (d - 1)) ** 2 for i in range(d)]
  return ls if metric == 0 else ls[::-1]


# -- problems and trials -------------------------------------------------------


def problem(space: str, n_metrics: int):
  from vizier_amd import pyvizier as vz
  p = vz.ProblemStatement()
  root = p.search_space.root
  if space == 'float':
    for i in range(4):
      root.add_float_param(f'x{i}', 0.0, 1.0)
  else:
    root.add_float_param('x0', 0.0, 1.0)
    root.add_int_param('k', 0, 3)
    root.add_float_param('x1', 0.0, 1.0)
    root.add_categorical_param('c', ['a', 'b', 'c'])
    root.add_float_param('x2', 0.0, 1.0)
  for m in range(n_metrics):
    p.metric_information.append(vz.MetricInformation(
        name=f'm{m}', goal=vz.ObjectiveMetricGoal.MAXIMIZE))
  return p


def _trials(space: str, n_metrics: int, n_pending: int, seed: int):
  """(completed, pending) trials with included coordinates in
  [TRIAL_LO, TRIAL_HI]."""
  from vizier_amd import pyvizier as vz
  rng = np.random.default_rng(seed)
  done, pending = [], []
  for uid in range(1, N_DONE + n_pending + 1):
    inc = rng.uniform(TRIAL_LO, TRIAL_HI, 4 if space == 'float' else 3)
    if space == 'float':
      params = {f'x{i}': float(v) for i, v in enumerate(inc)}
      extra = 0.0
    else:
      k, c = int(rng.integers(0, 2)), int(rng.integers(0, 2))
      params = {'x0': float(inc[0]), 'k': k, 'x1': float(inc[1]),
                'c': 'abc'[c], 'x2': float(inc[2])}
      extra = 0.05 * k - 0.04 * c
    t = vz.Trial(params, id=uid)
    if uid <= N_DONE:
      # Trial 1 is the clear best in every metric: the PE threshold is then
      # taken at row 0 whatever the rounding of the observed UCBs.
      bonus = 1.0 if uid == 1 else 0.0
      metrics = {'m0': float(-((inc - 0.2) ** 2).sum() + extra + bonus)}
      if n_metrics == 2:
        metrics['m1'] = float(inc.sum() - 2.0 * extra + 2.0 * bonus)
      t.complete(vz.Measurement(metrics=metrics))
      done.append(t)
    else:
      pending.append(t)
  return done, pending


def _raw(ls: List[float], extra=()) -> torch.Tensor:
  from vizier_amd._src.gp import gp_model as gm
  fb = gm._from_bounded
  head = [fb(math.log(AMP), *gm._LOG_AMP_BOUNDS),
          fb(math.log(NOISE), *gm._LOG_NOISE_BOUNDS),
          fb(MEAN_C, *gm._MEAN_BOUNDS)]
  tail = [fb(math.log(v), *gm._LOG_LS_BOUNDS) for v in ls]
  return torch.tensor(head + list(extra) + tail, dtype=torch.float32)


def installed_posterior(x: torch.Tensor, y: torch.Tensor, metric: int):
  from vizier_amd._src.gp import gp_model
  raw = _raw(lengthscales(x.shape[1], metric)).to(x.device)
  return gp_model._build_posterior_cache(x, y, raw, 0.0,
                                         precompute_inverse=True)


def installed_linear_posterior(x: torch.Tensor, y: torch.Tensor):
  """A LinearMaternPosterior at the same hyperparameters plus slope 0.3 and
  shift 0.2, cached as train_linear_matern_gp caches it (fp64, stored in
  x's dtype)."""
  from vizier_amd._src.gp import gp_model as gm
  from vizier_amd._src.gp import linear_matern as lm
  slope = gm._from_bounded(math.log(LIN_SLOPE), *gm._LOG_AMP_BOUNDS)
  raw = _raw(lengthscales(x.shape[1], 0), (slope, LIN_SHIFT)).to(x.device)
  p64 = lm.LinearMaternParams.from_raw(raw.double())
  n = x.shape[0]
  K = lm._combined_gram(p64, 1.0, x.double(), None)
  noise_eff = float(torch.maximum(p64.noise, 1e-3 * p64.amplitude ** 2))
  K = K + noise_eff * torch.eye(n, dtype=torch.float64, device=x.device)
  L = torch.linalg.cholesky(K)
  alpha = torch.cholesky_solve((y.double() - p64.mean).unsqueeze(-1), L)
  post = lm.LinearMaternPosterior(
      x=x, params=lm.LinearMaternParams.from_raw(raw), linear_coef=1.0,
      L=L.to(x.dtype), alpha=alpha.squeeze(-1).to(x.dtype), nll=0.0, raw=raw,
      noise_eff=noise_eff)
  return post


# -- designers ------------------------------------------------------------------


@dataclasses.dataclass
class Setup:
  designer: object
  space: str
  x_all: torch.Tensor              # the tensor the suggest loop would pass
  n_pending: int

  @property
  def device(self):
    return self.x_all.device


def ucbpe_setup(space: str, n_metrics: int, n_pending: int, device: str,
                **config) -> Setup:
  from vizier_amd._src.algorithms.core.abstractions import (
      ActiveTrials,
      CompletedTrials,
  )
  from vizier_amd._src.algorithms.designers.gp_ucb_pe import (
      UCBPEConfig,
      VizierGPUCBPEBandit,
  )
  d = VizierGPUCBPEBandit(problem(space, n_metrics), UCBPEConfig(
      ard_restarts=1, ard_max_iters=10, num_scalarizations=N_DIRECTIONS,
      device=device, **config), seed=1)
  done, pending = _trials(space, n_metrics, n_pending, seed=11)
  d.update(CompletedTrials(done), ActiveTrials(pending))
  d._fit()
  x = d._posterior.x
  labels = d._warped_labels
  if n_metrics == 2:
    d._mo_posteriors = [installed_posterior(x, labels[:, m], m)
                        for m in range(2)]
    d._posterior = d._mo_posteriors[0]
  elif config.get('mixes_linear_kernel'):
    d._posterior = installed_linear_posterior(x, labels)
  else:
    d._posterior = installed_posterior(x, labels, 0)
  x_all = x
  if pending:
    # As suggest() builds it.
    x_all = torch.cat([x, torch.as_tensor(
        d._converter.to_features(pending), dtype=d._config.dtype,
        device=d._device)], dim=0)
  return Setup(d, space, x_all, n_pending)


def bandit_setup(space: str, device: str, **config) -> Setup:
  from vizier_amd._src.algorithms.core.abstractions import (
      ActiveTrials,
      CompletedTrials,
  )
  from vizier_amd._src.algorithms.designers.gp_bandit import (
      GPBanditConfig,
      VizierGPBandit,
  )
  d = VizierGPBandit(problem(space, 2), GPBanditConfig(
      ard_restarts=1, ard_max_iters=10, num_scalarizations=N_DIRECTIONS,
      device=device, **config), seed=1)
  done, _ = _trials(space, 2, 0, seed=11)
  d.update(CompletedTrials(done), ActiveTrials())
  d._fit()
  d._posteriors = [installed_posterior(d._x, d._warped_labels[:, m], m)
                   for m in range(2)]
  return Setup(d, space, d._x, 0)


# -- candidates -----------------------------------------------------------------


@dataclasses.dataclass
class Candidates:
  dense: torch.Tensor          # (B, D) fp32 CPU feature rows
  continuous: torch.Tensor     # (B, 1, Dc) fp32 CPU
  categorical: torch.Tensor    # (B, 1, Dcat) int64 CPU
  close: torch.Tensor          # (B,) bool: excluded columns left at the row's

  def batch(self, device):
    from vizier_amd._src.algorithms.optimizers.eagle import CandidateBatch
    return CandidateBatch(self.continuous.to(device),
                          self.categorical.to(device))


def make_candidates(space: str, x_all: torch.Tensor, seed: int = 5
                    ) -> Candidates:
  """Rows [0, B/2): near a trusted row; rows [B/2, B): far from all.

  Mixed space, near candidates: trials only take k in {0, 1} and categories
  a, b, so a candidate with k in [0.85, 0.95] or with category c is at least
  0.5 from EVERY trusted row in an excluded column: there the posterior is
  back at its prior, sd is large and the PE penalty is off. Candidate q
  moves both (q % 4 == 1), only k (2) or only the category (3). `close` ones
  (q % 4 == 0, and q >= 12: near row 0 again or near a pending row) move
  neither: near the best trial, row 0, the penalty is off, near a trial
  with a low label it is on."""
  g = torch.Generator().manual_seed(seed)
  trusted = x_all.detach().cpu().double()
  mask = torch.tensor(MASKS[space], dtype=torch.bool)
  inc = (~mask).nonzero().flatten().tolist()
  d = len(mask)
  h = B // 2

  def r(*shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64)
  dense = torch.zeros(B, d, dtype=torch.float64)
  # Every trusted row (pending ones too) gets at least one near candidate.
  rows = torch.arange(h) % trusted.shape[0]
  # Offsets of 0.93 .. 0.99 NEAR in every included column: inside the radius,
  # yet far enough from the row for sd to clear the noise floor.
  sign = torch.where(r(h, len(inc)) < 0.5, -1.0, 1.0).double()
  near = trusted[rows][:, inc] + sign * NEAR * (0.93 + 0.06 * r(h, len(inc)))
  far = r(h, len(inc))
  for q in range(h):
    far[q, q % len(inc)] = FAR_LO + (1.0 - FAR_LO) * float(r(1))
  dense[:, inc] = torch.cat([near, far]).clamp(0.0, 1.0)
  cat = torch.zeros(B, 1, 0, dtype=torch.long)
  q = torch.arange(B)
  close = (q < h) & ((q % 4 == 0) | (q >= N_DONE))
  if space == 'mixed':
    move_k = ~close & (q % 4 != 2)
    move_c = ~close & (q % 4 != 3)
    k_row = torch.cat([trusted[rows][:, 1], r(h)])
    dense[:, 1] = torch.where(move_k, 0.85 + 0.1 * r(B), k_row + 0.05)
    c_row = torch.cat([trusted[rows][:, 3:6].argmax(-1),
                       torch.randint(2, (h,), generator=g)])
    c = torch.where(move_c, torch.full_like(c_row, 2), c_row)
    dense[:, 3:6] = torch.nn.functional.one_hot(c, 3).double()
    cat = c.reshape(B, 1, 1)
    cont_cols = [0, 1, 2, 6]
  else:
    cont_cols = [0, 1, 2, 3]
  dense = dense.float()
  return Candidates(dense, dense[:, cont_cols].unsqueeze(1).contiguous(), cat,
                    close)


# -- the fp64 view of a posterior ----------------------------------------------


@dataclasses.dataclass
class Post64:
  x: torch.Tensor
  ls: torch.Tensor
  amp: float
  mean_c: float
  alpha: torch.Tensor
  M: torch.Tensor                      # K_inv upcast, or (L L^T)^-1 from L
  slope: Optional[float] = None        # linear kernel: lc * slope, lc * shift
  shift: Optional[float] = None


def post64(p) -> Post64:
  def up(t):
    return t.detach().cpu().double()
  out = Post64(x=up(p.x), ls=up(p.params.lengthscales),
               amp=float(p.params.amplitude), mean_c=float(p.params.mean),
               alpha=up(p.alpha), M=None)
  if p.K_inv is not None:
    out.M = up(p.K_inv)
  else:
    L = up(p.L)
    out.M = torch.cholesky_inverse(L)
  if hasattr(p, 'linear_coef'):
    out.slope = p.linear_coef * float(p.params.slope)
    out.shift = p.linear_coef * float(p.params.shift)
  return out


@dataclasses.dataclass
class Pred:
  mean: torch.Tensor
  sd: torch.Tensor
  var: torch.Tensor
  d_mean: torch.Tensor
  d_sd: torch.Tensor
  d_var: torch.Tensor


def kvec(p: Post64, xq: torch.Tensor):
  """(k (B, N), prior (B,) or scalar) in fp64: Matern-5/2 (+ linear)."""
  z = (xq[:, None, :] - p.x[None, :, :]) / p.ls
  sr = sc.SQRT5 * (z * z).sum(-1).sqrt()
  k = p.amp ** 2 * (1.0 + sr + sr * sr / 3.0) * torch.exp(-sr)
  prior = torch.full((xq.shape[0],), p.amp ** 2, dtype=torch.float64)
  if p.slope is not None:
    zq, zx = xq / p.ls - p.shift, p.x / p.ls - p.shift
    k = k + p.slope ** 2 * (zq @ zx.T)
    prior = prior + p.slope ** 2 * (zq * zq).sum(-1)
  return k, prior


def predict(p: Post64, xq: torch.Tensor) -> Pred:
  n = p.x.shape[0]
  k, prior = kvec(p, xq)
  mean = p.mean_c + k @ p.alpha
  var = prior - ((k @ p.M) * k).sum(-1)
  sd = var.sqrt()
  d_mean = MARGIN * (K_REL + n * EPS32) * (k.abs() @ p.alpha.abs())
  d_var = MARGIN * (2.0 * K_REL + n * EPS32) * (
      prior + ((k.abs() @ p.M.abs()) * k.abs()).sum(-1))
  return Pred(mean, sd, var, d_mean, d_var / (2.0 * sd), d_var)


@dataclasses.dataclass
class LowpPred(Pred):
  emulation: tuple = ()


def predict_lowp(p, xq_dev: torch.Tensor, kind: str) -> Pred:
  """Mean / sd of posterior p (the designer's object, on its device) on the
  quantised operands of `kind`, with scorer_cases.lowp_bounds.

  fp8: Fp8GramCache, as the fused fp8 closure builds it. bf16: both sides
  (x / ls).to(bfloat16), as the gram_matern52_bf16 binding rounds them."""
  ls = p.params.lengthscales
  if kind == 'fp8':
    from vizier_amd._src.gp.acquisitions import Fp8GramCache
    cache = Fp8GramCache(p.x, ls, float(p.params.amplitude))
    z1q = gc.fp8_operand(xq_dev, ls, cache.scale)
    lo = dict(z1=(z1q.to(torch.float32) * cache.scale).cpu(),
              z2=cache.z2q.float().cpu(), n2=cache.n2.cpu(),
              scale=torch.tensor(cache.scale))
  else:
    z1b, z2b = gc.bf16_operands(xq_dev, p.x, ls)
    lo = dict(z1=z1b.float().cpu(), z2=z2b.float().cpu(),
              n2=gc.fp32_norms(z2b).cpu(), scale=torch.tensor(1.0))
  b, (n, d) = xq_dev.shape[0], p.x.shape
  case = sc.Case(b, n, d, p.x.cpu(), xq_dev.cpu(), ls.cpu(), p.alpha.cpu(),
                 p.K_inv.cpu())
  ref, tol_m, tol_q, emu = sc.lowp_bounds(case, lo)
  full = lambda v: torch.full((b,), v, dtype=torch.float64)
  return LowpPred(ref.mean, ref.sd, sc.AMP2 - ref.quad, full(tol_m),
                  full(tol_q) / (2.0 * ref.sd), full(tol_q), emu)


# -- scores ---------------------------------------------------------------------


@dataclasses.dataclass
class Scored:
  value: torch.Tensor                  # (B,) fp64
  tol: torch.Tensor                    # (B,) fp64
  penalised: Optional[torch.Tensor] = None   # (B,) bool: outside the radius
  dist: Optional[torch.Tensor] = None
  radius: float = 0.0
  info: dict = dataclasses.field(default_factory=dict)


def min_linf(xq: torch.Tensor, trusted: torch.Tensor, mask) -> torch.Tensor:
  return sc.min_linf_dist(xq, trusted, mask)


def trust(s: Scored, xq, trusted, mask, enabled: bool) -> Scored:
  """dist <= r ? score : -1e4 - dist, r from the number of trusted rows."""
  if not enabled:
    s.penalised = torch.zeros(xq.shape[0], dtype=torch.bool)
    return s
  r = radius(trusted.shape[0])
  assert r <= 0.5
  dist = min_linf(xq, trusted, mask)
  out = dist > r
  s.value = torch.where(out, -1e4 - dist, s.value)
  s.tol = torch.where(out, torch.full_like(s.tol, sc.TOL_PENALTY), s.tol)
  s.penalised, s.dist, s.radius = out, dist, r
  return s


def ucb(pred: Pred, coef: float) -> Scored:
  return Scored(pred.mean + coef * pred.sd,
                pred.d_mean + abs(coef) * pred.d_sd)


def threshold(p: Post64, coef: float):
  """Predicted mean at the observed point with the highest UCB; also its
  error bound and the gap to the runner-up UCB."""
  obs = predict(p, p.x)
  u = obs.mean + coef * obs.sd
  i = int(u.argmax())
  top = u.topk(2).values
  return (float(obs.mean[i]), float(obs.d_mean[i]), float(top[0] - top[1]),
          float((obs.d_mean + coef * obs.d_sd).max()))


def _penalty(explore, d_explore, thr, d_thr, pen_coef):
  gap = explore - thr
  slack = d_explore + d_thr
  return (pen_coef * gap.clamp_max(0.0),
          torch.where(gap <= slack, pen_coef * slack,
                      torch.zeros_like(slack)), gap)


def pe(post: Post64, var_post: Post64, xq, ucb_coef, explore_coef, pen_coef
       ) -> Scored:
  """stddev_all + pen * min(mean + c sd - thr, 0)."""
  pred, allp = predict(post, xq), predict(var_post, xq)
  thr, d_thr, gap_obs, tol_obs = threshold(post, ucb_coef)
  pen, d_pen, gap = _penalty(pred.mean + explore_coef * pred.sd,
                             pred.d_mean + explore_coef * pred.d_sd,
                             thr, d_thr, pen_coef)
  return Scored(allp.sd + pen, allp.d_sd + d_pen, info=dict(
      sd=pred.sd, sd_all=allp.sd, gap=gap, threshold=thr,
      obs_ucb_gap=gap_obs, obs_ucb_tol=tol_obs))


def hv(ys, d_ys, weights, ref):
  """mean_v min_m (y_m - ref_m) / w_vm and its bound. ys, d_ys: (B, M).

  Per direction: t_m the exact terms, e_m = d_y_m / w_m their error bounds,
  a = min_m t_m = t_m0, b = min_m t'_m = t'_m1 the perturbed minimum with
  |t'_m - t_m| <= e_m. Then b <= t'_m0 <= a + e_m0, and b = t'_m1 >=
  t_m1 - e_m1 >= a - e_m1, so |b - a| <= max(e_m0, e_m1). m0 is reachable
  (t_m0 - e_m0 <= t_m0 <= min_m (t_m + e_m)), and so is m1 (t_m1 - e_m1 <=
  t'_m1 = b <= min_m (t_m + e_m)); hence |b - a| <= max over the reachable
  m of e_m <= max_m d_y_m / min_m w_m, the plain bound."""
  v = weights.shape[0]
  t = (ys - ref)[None, :, :] / weights[:, None, :]          # (V, B, M)
  s = t.amin(-1)                                            # (V, B)
  # Only a metric whose lower end can undercut the smallest upper end can
  # become the argmin of the perturbed values; m = argmin is always one.
  e = d_ys[None, :, :] / weights[:, None, :]
  reachable = (t - e) <= (t + e).amin(-1, keepdim=True)
  d_s = torch.where(reachable, e, torch.zeros_like(e)).amax(-1) + \
      4.0 * EPS32 * s.abs()
  return s.mean(0), d_s.mean(0) + v * EPS32 * s.abs().mean(0)


def mo_scalarized(preds: List[Pred], coef, weights, ref):
  ys = torch.stack([p.mean + coef * p.sd for p in preds], -1)
  d_ys = torch.stack([p.d_mean + abs(coef) * p.d_sd for p in preds], -1)
  return hv(ys, d_ys, weights, ref)


def mo_ucb(preds: List[Pred], coef, weights, ref) -> Scored:
  return Scored(*mo_scalarized(preds, coef, weights, ref))


def mo_pe(posts: List[Post64], var_posts: List[Post64], xq, weights, ref,
          ucb_coef, explore_coef, pen_coef) -> Scored:
  """sum_m stddev_all_m + pen * min(HV(mean + c sd) - thr, 0), thr the
  scalarized mean at the observed point with the best scalarized UCB."""
  obs = [predict(p, posts[0].x) for p in posts]
  obs_ucb, d_obs_ucb = mo_scalarized(obs, ucb_coef, weights, ref)
  obs_mean, d_obs_mean = mo_scalarized(obs, 0.0, weights, ref)
  i = int(obs_ucb.argmax())
  top = obs_ucb.topk(2).values
  preds = [predict(p, xq) for p in posts]
  explore, d_explore = mo_scalarized(preds, explore_coef, weights, ref)
  pen, d_pen, gap = _penalty(explore, d_explore, float(obs_mean[i]),
                             float(d_obs_mean[i]), pen_coef)
  alls = [predict(vp, xq) for vp in var_posts]
  return Scored(sum(a.sd for a in alls) + pen,
                sum(a.d_sd for a in alls) + d_pen, info=dict(
                    sd=torch.stack([p.sd for p in preds]).amin(0),
                    sd_all=torch.stack([a.sd for a in alls]).amin(0),
                    gap=gap, threshold=float(obs_mean[i]),
                    obs_ucb_gap=float(top[0] - top[1]),
                    obs_ucb_tol=float(d_obs_ucb.max())))


def scalarizer_operands(setup: Setup):
  """(weights (V, M), reference point (M,)) in fp64, as the designer's
  scalarizer holds them (UCB-PE) or builds them per suggest (GP-Bandit)."""
  d = setup.designer
  s = getattr(d, '_mo_scalarizer', None)
  if s is None:
    from vizier_amd._src.gp import acquisitions as acq_lib
    s = acq_lib.create_hv_scalarization(
        d._config.num_scalarizations, 2, seed=d._seed,
        reference_point=acq_lib.get_reference_point(
            d._warped_labels, scale=d._config.ref_scaling))
  return (s.weights.detach().cpu().double(),
          s.reference_point.detach().cpu().double())


# -- one oracle per closure -------------------------------------------------------


def ucbpe_oracle(setup: Setup, cands: Candidates, use_ucb: bool,
                 swap_metrics=False, posterior_as_var_post=False) -> Scored:
  """The score VizierGPUCBPEBandit._one_score_fn(use_ucb, x_all) must give.

  swap_metrics / posterior_as_var_post build the deliberately WRONG oracles
  of the self-check."""
  d = setup.designer
  cfg = d._config
  xq = cands.dense.double()
  trusted = setup.x_all.detach().cpu().double()
  mask = MASKS[setup.space]
  mo = d._mo_posteriors is not None
  posts = list(d._mo_posteriors) if mo else [d._posterior]
  if swap_metrics:
    posts = posts[::-1]
  p64 = [post64(p) for p in posts]
  if use_ucb:
    preds = [predict(p, xq) for p in p64]
    if mo:
      s = mo_ucb(preds, cfg.ucb_coefficient, *scalarizer_operands(setup))
    else:
      s = ucb(preds[0], cfg.ucb_coefficient)
    s.info = dict(sd=torch.stack([p.sd for p in preds]).amin(0))
  else:
    if posterior_as_var_post:
      v64 = p64
    else:
      v64 = [post64(d._variance_posterior(setup.x_all, p)) for p in posts]
      assert all(v.x.shape[0] == trusted.shape[0] for v in v64)
    args = (cfg.ucb_coefficient, cfg.explore_region_ucb_coefficient,
            cfg.cb_violation_penalty_coefficient)
    if mo:
      s = mo_pe(p64, v64, xq, *scalarizer_operands(setup), *args)
    else:
      s = pe(p64[0], v64[0], xq, *args)
  return trust(s, xq, trusted, mask, cfg.use_trust_region)


def bandit_oracle(setup: Setup, cands: Candidates, swap_metrics=False
                  ) -> Scored:
  """The multi-objective score VizierGPBandit._score_factory(1) must give,
  for scorer_gram_dtype fp32 / fp8 / bf16."""
  d = setup.designer
  cfg = d._config
  posts = list(d._posteriors)
  if swap_metrics:
    posts = posts[::-1]
  xq = cands.dense.double()
  if cfg.scorer_gram_dtype == 'fp32':
    preds = [predict(post64(p), xq) for p in posts]
  else:
    xq_dev = cands.dense.to(setup.device)
    preds = [predict_lowp(p, xq_dev, cfg.scorer_gram_dtype) for p in posts]
  s = mo_ucb(preds, cfg.ucb_coefficient, *scalarizer_operands(setup))
  s.info = dict(sd=torch.stack([p.sd for p in preds]).amin(0),
                emulation=[getattr(p, 'emulation', ()) for p in preds])
  return trust(s, xq, d._x.detach().cpu().double(), MASKS[setup.space],
               cfg.use_trust_region)


# -- the rows of the test matrix ------------------------------------------------

# (id, designer, space, metrics, pending, use_ucb, config)
UCBPE_ROWS = [
    ('ucb-float', 'float', 1, 0, True, {}),
    ('ucb-mixed', 'mixed', 1, 0, True, {}),
    ('ucb-mixed-pending', 'mixed', 1, 2, True, {}),
    ('pe-mixed', 'mixed', 1, 0, False, {}),
    ('pe-mixed-pending', 'mixed', 1, 2, False, {}),
    ('pe-linear-pending', 'mixed', 1, 2, False,
     {'mixes_linear_kernel': True}),
    ('mo-ucb-float', 'float', 2, 0, True, {}),
    ('mo-ucb-mixed', 'mixed', 2, 0, True, {}),
    ('mo-ucb-mixed-pending', 'mixed', 2, 2, True, {}),
    ('mo-pe-mixed-pending', 'mixed', 2, 2, False, {}),
]
BANDIT_ROWS = [('bandit-mo-fp32', 'fp32'), ('bandit-mo-fp8', 'fp8'),
               ('bandit-mo-bf16', 'bf16')]


@functools.lru_cache(maxsize=None)
def ucbpe_case(row: str, trust_region: bool, device: str):
  """(setup, candidates, use_ucb) of a UCBPE_ROWS id: built once per
  process and never mutated."""
  _, space, n_metrics, n_pending, use_ucb, config = next(
      r for r in UCBPE_ROWS if r[0] == row)
  setup = ucbpe_setup(space, n_metrics, n_pending, device,
                      use_trust_region=trust_region, **config)
  return setup, make_candidates(space, setup.x_all), use_ucb


@functools.lru_cache(maxsize=None)
def bandit_case(gram_dtype: str, trust_region: bool, device: str):
  setup = bandit_setup('mixed', device, scorer_gram_dtype=gram_dtype,
                       use_trust_region=trust_region)
  return setup, make_candidates('mixed', setup.x_all)
