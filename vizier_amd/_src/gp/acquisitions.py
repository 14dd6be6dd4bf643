"""Acquisition functions + trust region (PyTorch).

Capability parity with vizier/_src/algorithms/designers/gp/acquisitions.py
(UCB :214 w/ default coef 1.8, LCB :229, EI :244, PI :261, Sample :278,
q-family :496-569, create_hv_scalarization :571, TrustRegion :691-820
with the -1e4-distance outside-penalty :152-174).
"""

from __future__ import annotations

import dataclasses
import math
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from vizier_amd._src.gp.gp_model import GPPosterior


def _normal():
  return torch.distributions.Normal(0.0, 1.0)


class AcquisitionFunction:
  """Maps posterior (mean, stddev) at candidates to scores."""

  def __call__(self, mean: torch.Tensor, stddev: torch.Tensor
               ) -> torch.Tensor:
    raise NotImplementedError


@dataclasses.dataclass
class UCB(AcquisitionFunction):
  coefficient: float = 1.8

  def __call__(self, mean, stddev):
    return mean + self.coefficient * stddev


@dataclasses.dataclass
class LCB(AcquisitionFunction):
  coefficient: float = 1.8

  def __call__(self, mean, stddev):
    return mean - self.coefficient * stddev


@dataclasses.dataclass
class EI(AcquisitionFunction):
  """Expected improvement over `best_value` (labels are maximized)."""

  best_value: float = 0.0

  def __call__(self, mean, stddev):
    z = (mean - self.best_value) / stddev
    n = _normal()
    return stddev * (z * n.cdf(z) + n.log_prob(z).exp())


@dataclasses.dataclass
class PI(AcquisitionFunction):
  best_value: float = 0.0

  def __call__(self, mean, stddev):
    z = (mean - self.best_value) / stddev
    return _normal().cdf(z)


@dataclasses.dataclass
class Sample(AcquisitionFunction):
  """Thompson-style single posterior sample."""

  seed: int = 0

  def __call__(self, mean, stddev):
    g = torch.Generator(device='cpu').manual_seed(self.seed)
    eps = torch.randn(mean.shape, generator=g).to(mean.device, mean.dtype)
    return mean + stddev * eps


class MaxValueEntropySearch(AcquisitionFunction):
  """MES (acquisitions.py:293), Gumbel-sampled max-value approximation.

  score(x) = mean over sampled maxima y* of
      gamma * pdf(gamma) / (2 cdf(gamma)) - log cdf(gamma),
  gamma = (y* - mu) / sigma (Wang & Jegelka 2017).
  """

  def __init__(self, best_value: float = 0.0, num_max_samples: int = 16,
               max_value_spread: float = 1.0, seed: int = 0):
    self.best_value = best_value
    self.num_max_samples = num_max_samples
    self.max_value_spread = max_value_spread
    self.seed = seed

  def __call__(self, mean, stddev):
    g = torch.Generator(device='cpu').manual_seed(self.seed)
    # Gumbel samples of the global max, anchored above the incumbent.
    u = torch.rand(self.num_max_samples, generator=g).clamp(1e-6,
                                                            1 - 1e-6)
    # The global max is at least the incumbent: clamp the Gumbel tail.
    gumbel = (-torch.log(-torch.log(u))).clamp_min(0.0) * 0.25 * \
        self.max_value_spread
    y_star = (self.best_value + 0.05 * self.max_value_spread +
              gumbel).to(mean.device, mean.dtype)
    n = _normal()
    gamma = (y_star.reshape(-1, 1) - mean.unsqueeze(0)) / stddev
    cdf = n.cdf(gamma).clamp_min(1e-9)
    pdf = n.log_prob(gamma).exp()
    return (gamma * pdf / (2.0 * cdf) - torch.log(cdf)).mean(0)


# -- q-family: joint acquisition of a parallel suggestion batch -------------


def _posterior_samples(posterior: GPPosterior, xq: torch.Tensor,
                       num_samples: int, seed: int) -> torch.Tensor:
  """(S, Q) joint samples of f at xq (uses the full predictive cov)."""
  mean, cov = posterior.predict_cov(xq)
  q = xq.shape[0]
  cov = cov + 1e-8 * torch.eye(q, dtype=cov.dtype, device=cov.device)
  L = torch.linalg.cholesky(cov)
  g = torch.Generator(device='cpu').manual_seed(seed)
  eps = torch.randn(num_samples, q, generator=g).to(mean.device, mean.dtype)
  return mean.unsqueeze(0) + eps @ L.T


@dataclasses.dataclass
class QEI:
  """Monte-Carlo q-EI: mean over samples of max-improvement in the batch."""

  best_value: float = 0.0
  num_samples: int = 128
  seed: int = 0

  def __call__(self, posterior: GPPosterior, xq: torch.Tensor
               ) -> torch.Tensor:
    samples = _posterior_samples(posterior, xq, self.num_samples, self.seed)
    improvement = (samples - self.best_value).clamp_min(0.0)
    return improvement.amax(dim=1).mean()


@dataclasses.dataclass
class QPI:
  best_value: float = 0.0
  num_samples: int = 128
  seed: int = 0

  def __call__(self, posterior, xq):
    samples = _posterior_samples(posterior, xq, self.num_samples, self.seed)
    return (samples.amax(dim=1) > self.best_value).float().mean()


@dataclasses.dataclass
class QUCB:
  """q-UCB via |deviation| trick: mean + c * sqrt(pi/2) |eps| stddev."""

  coefficient: float = 1.8
  num_samples: int = 128
  seed: int = 0

  def __call__(self, posterior, xq):
    mean, cov = posterior.predict_cov(xq)
    q = xq.shape[0]
    cov = cov + 1e-8 * torch.eye(q, dtype=cov.dtype, device=cov.device)
    L = torch.linalg.cholesky(cov)
    g = torch.Generator(device='cpu').manual_seed(self.seed)
    eps = torch.randn(self.num_samples, q, generator=g).to(mean.device,
                                                           mean.dtype)
    dev = (eps @ L.T).abs() * math.sqrt(math.pi / 2.0)
    return (mean.unsqueeze(0) + self.coefficient * dev).amax(dim=1).mean()


# -- scalarization (multi-objective) ----------------------------------------


@dataclasses.dataclass
class HyperVolumeScalarization:
  """Chebyshev-style hypervolume scalarization (acquisitions.py:571).

  score(y) = min_m (y_m - ref_m)/w_m over positive weights w.
  """

  weights: torch.Tensor      # (V, M) positive directions
  reference_point: Optional[torch.Tensor] = None  # (M,)

  def __call__(self, ys: torch.Tensor) -> torch.Tensor:
    """ys: (..., M) -> (V, ...) scalarized values."""
    if self.weights.device != ys.device:
      self.weights = self.weights.to(ys.device, ys.dtype)
      if self.reference_point is not None:
        self.reference_point = self.reference_point.to(ys.device, ys.dtype)
    if self.reference_point is not None:
      ys = ys - self.reference_point
    w = self.weights.reshape((-1,) + (1,) * (ys.dim() - 1) + (ys.shape[-1],))
    return (ys.unsqueeze(0) / w).amin(dim=-1)


def create_hv_scalarization(num_scalarizations: int, num_metrics: int,
                            seed: int = 0,
                            reference_point: Optional[torch.Tensor] = None
                            ) -> HyperVolumeScalarization:
  g = torch.Generator(device='cpu').manual_seed(seed)
  w = torch.randn(num_scalarizations, num_metrics, generator=g).abs()
  w = w / w.norm(dim=-1, keepdim=True)
  return HyperVolumeScalarization(weights=w.clamp_min(1e-6),
                                  reference_point=reference_point)


def get_reference_point(labels: torch.Tensor, scale: float = 0.01
                        ) -> torch.Tensor:
  """worst - scale * range per metric (acquisitions.py:~130)."""
  best = labels.amax(dim=0)
  worst = labels.amin(dim=0)
  return worst - scale * (best - worst)


# -- trust region ------------------------------------------------------------


def converter_trust_masks(converter) -> tuple:
  """(exclude_mask list[bool] over feature columns, n_categorical_params).

  Mirrors the reference's TrustRegion.__post_init__ dimension masking
  (acquisitions.py:736-749): a continuified discrete/integer column is
  excluded when its feasible values, scaled to [0,1], have a consecutive
  gap > min_radius (0.2), or when it has a single feasible value.
  """
  from vizier_amd import pyvizier as vz
  min_radius = TrustRegion.MIN_RADIUS
  exclude = [False] * converter.n_features
  n_cat = 0
  for col in converter.output_specs:
    if col.is_onehot:
      n_cat += 1
      for c in range(col.start, col.start + col.width):
        exclude[c] = True
      continue
    cfg = col.config
    if cfg.type in (vz.ParameterType.DISCRETE, vz.ParameterType.INTEGER):
      lo, hi = cfg.bounds
      if hi == lo:
        exclude[col.start] = True
        continue
      if cfg.type == vz.ParameterType.DISCRETE:
        vals = sorted(float(v) for v in cfg.feasible_values)
      else:
        # Integers: enumerate when small; for wide ranges the largest
        # scaled gap is between the two lowest values under LOG scaling
        # (linear spacing is uniform), so those two suffice.
        if hi - lo <= 64:
          vals = [float(v) for v in range(int(lo), int(hi) + 1)]
        else:
          vals = [float(lo), float(lo) + 1.0, float(hi)]
      if len(vals) < 2:
        exclude[col.start] = True
        continue
      scaled = [_scale_value(cfg, v) for v in vals]
      max_gap = max(b - a for a, b in zip(scaled[:-1], scaled[1:]))
      if max_gap > min_radius:
        exclude[col.start] = True
  return exclude, n_cat


def _scale_value(cfg, value: float) -> float:
  """[0,1] scaling consistent with converters.core._scale."""
  import math
  lo, hi = cfg.bounds
  if hi == lo:
    return 0.0
  st = cfg.scale_type
  from vizier_amd import pyvizier as vz
  if st == vz.ScaleType.LOG and lo > 0:
    return (math.log(value) - math.log(lo)) / (math.log(hi) - math.log(lo))
  if st == vz.ScaleType.REVERSE_LOG and lo > 0:
    flipped = hi + lo - value
    return 1.0 - (math.log(flipped) - math.log(lo)) / (
        math.log(hi) - math.log(lo))
  return (value - lo) / (hi - lo)


class TrustRegion:
  """Union of L-inf balls around observed points (acquisitions.py:691).

  radius = 0.2 + (0.5 - 0.2) * num_obs / (5 * (dof + 1)); a radius > 0.5
  disables the constraint. Matches the reference's dof accounting
  (acquisitions.py:752-768): dof = number of continuous feature columns
  participating in the distance + ONE per categorical parameter (not one
  per one-hot column). Columns flagged in `onehot_column_mask` — one-hot
  blocks plus wide-gap discretes excluded via `for_converter` — are
  excluded from the L-inf distance.
  """

  MIN_RADIUS = 0.2
  DIMENSION_FACTOR = 5.0

  def __init__(self, trusted: torch.Tensor,
               onehot_column_mask: Optional[torch.Tensor] = None,
               *, n_categorical_params: Optional[int] = None):
    """trusted: (N, D) observed features in [0,1]."""
    self._trusted = trusted
    d = trusted.shape[-1]
    if onehot_column_mask is None:
      onehot_column_mask = torch.zeros(d, dtype=torch.bool,
                                       device=trusted.device)
    self._onehot = onehot_column_mask
    n_excluded = int(onehot_column_mask.sum())
    if n_categorical_params is None:
      # Fallback when built from a bare mask: each contiguous run of
      # excluded columns is treated as one categorical parameter's
      # one-hot block.
      m = onehot_column_mask.to('cpu', torch.int8)
      n_categorical_params = int(
          ((m[1:] - m[:-1]) == 1).sum() + (1 if d and m[0] else 0))
    num_obs = trusted.shape[0]
    dof = (d - n_excluded) + n_categorical_params
    trust_level = num_obs / (self.DIMENSION_FACTOR * (dof + 1))
    if num_obs == 0:
      self.trust_radius = 1.0
    else:
      self.trust_radius = self.MIN_RADIUS + (0.5 - self.MIN_RADIUS) * \
          trust_level

  @classmethod
  def for_converter(cls, trusted: torch.Tensor, converter
                    ) -> 'TrustRegion':
    """Builds the reference-faithful region from a TrialToArrayConverter.

    Excludes from the distance: one-hot blocks, single-value parameters,
    and continuified discrete/integer parameters whose largest gap
    between consecutive scaled feasible values exceeds MIN_RADIUS
    (reference acquisitions.py:736-749 `_continuous_dimensions_mask`).
    """
    mask, n_cat = converter_trust_masks(converter)
    return cls(trusted,
               torch.as_tensor(mask, device=trusted.device),
               n_categorical_params=n_cat)

  def min_linf_distance(self, xs: torch.Tensor) -> torch.Tensor:
    """xs: (..., D) -> (...) L-inf distance to the nearest trusted point."""
    if self._trusted.shape[0] == 0:
      return torch.full(xs.shape[:-1], -float('inf'), dtype=xs.dtype,
                        device=xs.device)
    diff = (xs.unsqueeze(-2) - self._trusted).abs()   # (..., N, D)
    diff = torch.where(self._onehot, torch.zeros_like(diff), diff)
    return diff.amax(dim=-1).amin(dim=-1)

  def apply(self, xs: torch.Tensor, scores: torch.Tensor) -> torch.Tensor:
    """Penalizes scores outside the region: -1e4 - distance."""
    if self.trust_radius > 0.5:
      return scores
    distance = self.min_linf_distance(xs)
    return torch.where(distance <= self.trust_radius, scores,
                       -1e4 - distance)


class Fp8GramCache:
  """Per-posterior fp8 operand cache for candidate cross-grams.

  Hoists the training-side quantization (and the range-scan host sync)
  out of the sweep loop: the scale is the deterministic unit-box bound
  s = max_d(1/ls_d)/8 (all features live in [0,1], so every candidate
  and training row satisfies |z|/s <= 8 — comfortably inside e4m3).
  `gram(xs)` is then conversion-light, sync-free and capture-safe.
  """

  def __init__(self, x: torch.Tensor, lengthscales: torch.Tensor,
               amplitude: float):
    self.ls = lengthscales
    self.amp = float(amplitude)
    self.scale = max(float((1.0 / lengthscales).max()) / 8.0, 1e-8)
    d = x.shape[1]
    self.dp = (d + 31) // 32 * 32
    z = x / lengthscales
    z2q = torch.zeros(x.shape[0], self.dp,
                      dtype=torch.float8_e4m3fn, device=x.device)
    z2q[:, :d] = (z / self.scale).to(torch.float8_e4m3fn)
    self.z2q = z2q
    z2f = z2q.to(torch.float32) * self.scale
    self.n2 = (z2f * z2f).sum(-1)

  def gram(self, xs: torch.Tensor) -> torch.Tensor:
    from vizier_amd._src.ops import dispatch as ops
    ext = ops.require_ext()
    d = xs.shape[1]
    z1 = xs / self.ls
    z1q = torch.zeros(xs.shape[0], self.dp,
                      dtype=torch.float8_e4m3fn, device=xs.device)
    z1q[:, :d] = (z1 / self.scale).to(torch.float8_e4m3fn)
    z1f = z1q.to(torch.float32) * self.scale
    n1 = (z1f * z1f).sum(-1)
    return ext.gram_matern52_fp8_pre(z1q, self.z2q, n1, self.n2,
                                     self.amp, self.scale)


def bf16_train_operands(x: torch.Tensor, lengthscales: torch.Tensor
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
  """Training-side operands of the fused bf16 scorer, built once per suggest.

  Returns (z2b, n2): z2b (N, Dp) = bf16(x / lengthscales), zero-padded to
  a multiple of 32 columns, and n2 (N,) = fp32 row norms of the ROUNDED
  values (the layout ext.posterior_scores_bf16 consumes).
  """
  with torch.no_grad():
    z = x / lengthscales
    d = z.shape[1]
    dp = (d + 31) // 32 * 32
    z2b = torch.zeros(z.shape[0], dp, dtype=torch.bfloat16,
                      device=z.device)
    z2b[:, :d] = z.to(torch.bfloat16)
    n2 = (z2b.float() ** 2).sum(-1)
  return z2b, n2


def qei_mc_scores(mean: torch.Tensor, cov: torch.Tensor,
                  eps: torch.Tensor, best_value: float) -> torch.Tensor:
  """Monte-Carlo qEI over candidate SETS with common random numbers.

  mean (B, q), cov (B, q, q), eps (S, q) iid N(0,1) draws ->
  scores (B,): E_s[ max_q (mean + L eps_s - best)_+ ] with
  L = chol(cov + jitter); batch elements whose covariance still fails
  to factor fall back to independent marginals (diagonal L).
  Correlated sampling uses y = L @ eps (covariance L L^T = cov);
  the transposed product L^T eps has covariance L^T L — wrong marginals
  AND wrong correlations for q > 1 (regression-tested).
  """
  B, q = mean.shape
  eye = torch.eye(q, dtype=cov.dtype, device=cov.device)
  diag = cov.diagonal(dim1=-2, dim2=-1)
  jitter = 1e-4 * diag.mean(-1, keepdim=True).clamp_min(1e-10)
  cov = cov + jitter.unsqueeze(-1) * eye
  L, info = torch.linalg.cholesky_ex(cov)          # (B, q, q)
  bad = (info > 0)
  L_diag = torch.diag_embed(diag.clamp_min(1e-12).sqrt())
  L = torch.where(bad.view(-1, 1, 1), L_diag, L)
  # y[s, b, r] = mean[b, r] + sum_c L[b, r, c] * eps[s, c]
  samples = mean.unsqueeze(0) + torch.einsum(
      'sc,brc->sbr', eps, L)
  return (samples - best_value).clamp_min(0).amax(-1).mean(0)


class QEISetScoringFunction:
  """Monte-Carlo qEI over candidate sets as one fused HIP op (GPU, fp32).

  dense (B, q <= 16, D) -> (B,): `posterior_batched_cov` + `qei_mc_scores`
  + `TrustRegion.apply(dense[:, 0, :], .)` computed by qei_score.hip
  (k-vectors, one K^-1 SGEMM, joint covariance, q x q Cholesky with the
  diagonal fallback, max-improvement over the common draws `eps` (S, q)).
  No host sync per call, so the sweep can capture it in a hipGraph.
  Needs a plain GPPosterior with K_inv and a trust region anchored at the
  posterior's training points.
  """

  def __init__(self, posterior: GPPosterior, eps: torch.Tensor,
               best_value: float,
               trust_region: Optional[TrustRegion] = None):
    if posterior.K_inv is None:
      raise ValueError('QEISetScoringFunction needs a posterior with K_inv')
    if trust_region is not None and not (
        trust_region._trusted.shape == posterior.x.shape and
        trust_region._trusted.data_ptr() == posterior.x.data_ptr()):
      raise ValueError('QEISetScoringFunction needs a trust region '
                       'anchored at the posterior training points')
    self.posterior = posterior
    self.trust_region = trust_region
    self.eps = eps.contiguous()
    # Pre-extract scalars once so the hot loop never syncs the device.
    self._amp = float(posterior.params.amplitude)
    self._mean_c = float(posterior.params.mean)
    self._best = float(best_value)
    d = posterior.x.shape[-1]
    if trust_region is not None:
      self._onehot_u8 = trust_region._onehot.to(torch.uint8)
      self._tr_radius = float(trust_region.trust_radius)
    else:
      self._onehot_u8 = torch.zeros(d, dtype=torch.uint8,
                                    device=posterior.x.device)
      self._tr_radius = 0.0

  def __call__(self, dense: torch.Tensor) -> torch.Tensor:
    from vizier_amd._src.ops import dispatch as ops
    post = self.posterior
    return ops.require_ext().qei_set_scores(
        dense, post.x, post.params.lengthscales, self._amp, self._mean_c,
        post.alpha, post.K_inv, self._onehot_u8, self.eps, self._best,
        self._tr_radius)


class SetPEScoringFunction:
  """GP-UCB-PE set-PE score over candidate sets as one fused HIP op.

  dense (B, q <= 16, D) -> (B,), GPU and fp32 only:
      logdet(cov(set | var_posterior) + 1e-10 amp^2 I)
      + penalty_coef * sum_q min(explore_ucb(x_q) - threshold, 0)
      + sum_q [dist_q > radius] (-1e4 - dist_q)
  with explore_ucb = mean + explore_coef * stddev under `posterior` (the
  completed trials) and the covariance and trust-region distances under
  `var_posterior` (completed + pending; only its variance is used). A set
  whose jittered covariance is not positive definite scores -inf. The
  k-vector, K^-1 and covariance kernels are those of the qEI scorer;
  setpe_score.hip adds the one-wave Cholesky logdet tail. No host sync per
  call, so the sweep can capture it in a hipGraph. Needs plain
  GPPosteriors with K_inv and a trust region anchored at var_posterior.x.
  """

  def __init__(self, posterior: GPPosterior, var_posterior: GPPosterior,
               threshold: float, explore_coef: float, penalty_coef: float,
               trust_region: Optional[TrustRegion] = None):
    for name, post in (('posterior', posterior),
                       ('var_posterior', var_posterior)):
      if type(post) is not GPPosterior:
        raise ValueError(f'SetPEScoringFunction needs a plain GPPosterior '
                         f'as {name}, got {type(post).__name__}')
      if post.K_inv is None:
        raise ValueError(
            f'SetPEScoringFunction needs a {name} with K_inv')
    if trust_region is not None and not (
        trust_region._trusted.shape == var_posterior.x.shape and
        trust_region._trusted.data_ptr() == var_posterior.x.data_ptr()):
      raise ValueError('SetPEScoringFunction needs a trust region '
                       'anchored at var_posterior.x')
    self.posterior = posterior
    self.var_posterior = var_posterior
    self.trust_region = trust_region
    # Pre-extract scalars once so the hot loop never syncs the device.
    self._amp = float(var_posterior.params.amplitude)
    self._mean_c = float(posterior.params.mean)
    self._threshold = float(threshold)
    self._explore_coef = float(explore_coef)
    self._penalty_coef = float(penalty_coef)
    d = posterior.x.shape[-1]
    if trust_region is not None:
      self._onehot_u8 = trust_region._onehot.to(torch.uint8)
      self._tr_radius = float(trust_region.trust_radius)
    else:
      self._onehot_u8 = torch.zeros(d, dtype=torch.uint8,
                                    device=posterior.x.device)
      self._tr_radius = 0.0

  def __call__(self, dense: torch.Tensor) -> torch.Tensor:
    from vizier_amd._src.ops import dispatch as ops
    post, var_post = self.posterior, self.var_posterior
    return ops.require_ext().setpe_set_scores(
        dense, post.x, post.alpha, post.K_inv, self._mean_c, var_post.x,
        var_post.K_inv, var_post.params.lengthscales, self._amp,
        self._onehot_u8, self._threshold, self._explore_coef,
        self._penalty_coef, self._tr_radius)


class ScoringFunction:
  """Posterior + acquisition + optional trust region, over a batch.

  The callable the acquisition optimizer evaluates: xs (B, D) -> (B,).
  On GPU (with the trust region anchored at the training points, the
  GP-Bandit case) this is ONE fused HIP launch (posterior_score.hip);
  otherwise it composes torch ops.
  """

  _FUSED = {UCB: 'ucb', LCB: 'lcb', EI: 'ei', PI: 'pi'}

  def __init__(self, posterior: GPPosterior,
               acquisition: AcquisitionFunction,
               trust_region: Optional[TrustRegion] = None,
               gram_dtype: str = 'fp32'):
    self.posterior = posterior
    self.acquisition = acquisition
    self.trust_region = trust_region
    # 'fp32' (default) | 'bf16' | 'fp8': compute dtype for the
    # candidate k-vector Gram in the COMPOSED path (bf16/fp8 MFMA
    # kernels; configs 2/5 of BASELINE.json). The fused chunked kernel
    # stays fp32, so a non-fp32 gram_dtype forces the composed path.
    self.gram_dtype = gram_dtype
    # Pre-extract scalars once so the hot loop never syncs the device.
    self._amp = float(posterior.params.amplitude)
    self._mean_c = float(posterior.params.mean)
    self._acq_name = self._FUSED.get(type(acquisition))
    self._coef = getattr(acquisition, 'coefficient', 0.0)
    self._best = getattr(acquisition, 'best_value', 0.0)
    self._onehot_u8 = None
    # bf16 fused path: cache the TRAINING-side operands once per
    # suggest (z2b = bf16(x / lengthscales), n2 = rounded row norms);
    # the HIP kernel then only rounds the 25 candidates per iteration,
    # so the bf16 scorer is a 3-launch graph-capturable sequence like
    # fp32 instead of ~15 eager conversion launches.
    self._bf16_cache = None
    self._fp8_cache = None
    if (gram_dtype == 'fp8' and posterior.x.is_cuda and
        posterior.K_inv is not None):
      self._fp8_cache = Fp8GramCache(posterior.x,
                                     posterior.params.lengthscales,
                                     float(posterior.params.amplitude))
    if (gram_dtype == 'bf16' and posterior.x.is_cuda and
        posterior.K_inv is not None and self._acq_name is not None):
      self._bf16_cache = bf16_train_operands(
          posterior.x, posterior.params.lengthscales)
    if trust_region is not None:
      self._onehot_u8 = trust_region._onehot.to(torch.uint8)
      self._tr_radius = float(trust_region.trust_radius)
      trusted = trust_region._trusted
      self._tr_anchored = (
          trusted.shape == posterior.x.shape and
          trusted.data_ptr() == posterior.x.data_ptr())
    else:
      self._tr_radius = 0.0
      self._tr_anchored = True

  def _can_fuse(self, xs: torch.Tensor) -> bool:
    """True when the GPU K^-1 quadform path applies (any acquisition).

    fp32 always; float64 (parity mode) only with VIZIER_AMD_FP64_HIP=1,
    otherwise it scores through the torch predict path (rocBLAS DGEMM).
    """
    if self.posterior.K_inv is None or not xs.is_cuda:
      return False
    if xs.dtype == torch.float32:
      return True
    from vizier_amd._src.ops import dispatch as ops
    return ops.use_fp64_hip(xs) and ops.use_fp64_hip(self.posterior.x)

  def _call_fp64_hip(self, xs: torch.Tensor) -> torch.Tensor:
    """float64 on the GPU with VIZIER_AMD_FP64_HIP=1 (see _can_fuse)."""
    post = self.posterior
    from vizier_amd._src.ops import dispatch as ops
    if (self._acq_name is not None and self._tr_anchored and
        self.gram_dtype == 'fp32'):
      # The 3-kernel fp64 scorer (posterior_score_f64.hip): k-vectors,
      # K^-1 quadform on the fp64 matrix cores, finalize. No host sync,
      # so the sweep captures it in a hipGraph like the fp32 scorer.
      onehot = self._onehot_u8
      if onehot is None:
        onehot = torch.zeros(xs.shape[-1], dtype=torch.uint8,
                             device=xs.device)
        self._onehot_u8 = onehot
      ext = ops.require_ext()
      return ext.posterior_scores_f64(
          xs, post.x, post.params.lengthscales, self._amp, self._mean_c,
          post.alpha, post.K_inv, onehot, ops.ACQ_CODES[self._acq_name],
          self._coef, self._best,
          self._tr_radius if self.trust_region is not None else 0.0)
    # Composed path (exotic acquisition, unanchored trust region, or a
    # low-precision gram_dtype, which has no fp64 form): fp64 HIP Gram
    # for the k-vectors + rocBLAS DGEMM for the quadform.
    k = ops.gram_matern52(xs, post.x, post.params.lengthscales,
                          post.params.amplitude)
    amp2 = self._amp * self._amp
    var = (amp2 - (k * (k @ post.K_inv)).sum(-1)).clamp_min(1e-12)
    mean = self._mean_c + k @ post.alpha
    scores = self.acquisition(mean, var.sqrt())
    if self.trust_region is not None:
      scores = self.trust_region.apply(xs, scores)
    return scores

  def __call__(self, xs: torch.Tensor) -> torch.Tensor:
    if self._can_fuse(xs):
      post = self.posterior
      from vizier_amd._src.ops import dispatch as ops
      if xs.dtype == torch.float64:
        return self._call_fp64_hip(xs)
      if (self._acq_name is not None and self._tr_anchored and
          self._bf16_cache is not None):
        # bf16 fused scorer: cached training operands, 3 launches.
        onehot = self._onehot_u8
        if onehot is None:
          onehot = torch.zeros(xs.shape[-1], dtype=torch.uint8,
                               device=xs.device)
          self._onehot_u8 = onehot
        z2b, n2 = self._bf16_cache
        ext = ops.require_ext()
        return ext.posterior_scores_bf16(
            xs, post.x, z2b, n2, post.params.lengthscales, self._amp,
            self._mean_c, post.alpha, post.K_inv, onehot,
            ops.ACQ_CODES[self._acq_name], self._coef, self._best,
            self._tr_radius if self.trust_region is not None else 0.0)
      if (self._acq_name is not None and self._tr_anchored and
          self.gram_dtype == 'fp32'):
        # Primary GPU path: the 3-kernel chunked HIP scorer — one
        # Python op; k-vectors + chip-filling K^-1 quadform chunks +
        # acquisition/trust-region finalize (posterior_score.hip).
        onehot = self._onehot_u8
        if onehot is None:
          onehot = torch.zeros(xs.shape[-1], dtype=torch.uint8,
                               device=xs.device)
          self._onehot_u8 = onehot
        ext = ops.require_ext()
        return ext.posterior_scores_chunked(
            xs, post.x, post.params.lengthscales, self._amp,
            self._mean_c, post.alpha, post.K_inv, onehot,
            ops.ACQ_CODES[self._acq_name], self._coef, self._best,
            self._tr_radius if self.trust_region is not None else 0.0)
      # Composed path: hand-written HIP gram kernel for the k-vectors +
      # rocBLAS for the plain K^-1 quadform GEMM (used for exotic
      # acquisitions / unanchored trust regions / bf16+fp8 grams).
      ext = ops.require_ext()
      if self.gram_dtype == 'bf16':
        k = ext.gram_matern52_bf16(xs, post.x, post.params.lengthscales,
                                   float(post.params.amplitude))
      elif self.gram_dtype == 'fp8':
        if self._fp8_cache is not None:
          # Cached training-side operands: no per-call range scan
          # (host sync) or conversions (see Fp8GramCache).
          k = self._fp8_cache.gram(xs)
        else:
          k = ext.gram_matern52_fp8(xs, post.x,
                                    post.params.lengthscales,
                                    float(post.params.amplitude))
      else:
        k = ops.gram_matern52(xs, post.x, post.params.lengthscales,
                              post.params.amplitude)
      amp2 = self._amp * self._amp
      var = (amp2 - (k * (k @ post.K_inv)).sum(-1)).clamp_min(1e-12)
      mean = self._mean_c + k @ post.alpha
      scores = self.acquisition(mean, var.sqrt())
      if self.trust_region is not None:
        scores = self.trust_region.apply(xs, scores)
      return scores
    mean, stddev = self.posterior.predict(xs)
    scores = self.acquisition(mean, stddev)
    if self.trust_region is not None:
      scores = self.trust_region.apply(xs, scores)
    return scores
