"""Operands and fp64 references for the fused set-PE scorer (setpe_score.hip).

GP-UCB-PE scores a set of q exploration candidates by

    logdet(cov(set | completed + pending) + 1e-10 amp^2 I)
    + penalty_coef * sum_q min(explore_ucb(x_q) - threshold, 0)
    + sum_q [dist_q > radius] (-1e4 - dist_q)

with explore_ucb = mean + explore_coef * stddev under the completed-trials
posterior. A case is therefore TWO real GPs built in fp64 the way
tests/qei_cases.py builds one: `explore` over x (N rows) and `var` over
x_all = cat(x, pending) (N + P rows; P = 0 means x_all is x), same
lengthscales, amplitude and noise, alpha = 0 for `var` (only its variance is
used). Both are qei_cases.Case objects over the same candidate sets, so the
qEI helpers (posterior, joint_reference, joint_bounds) apply to each. Every
operand is rounded to fp32 ONCE; the fp64 reference runs on the `.double()`
images. threshold = the median of the reference explore_ucb, so about half
the members are penalised.

The reference is the production torch code of
VizierGPUCBPEBandit._set_pe_score_fn (GPPosterior.predict,
gp_bandit.posterior_batched_cov, torch.linalg.cholesky_ex,
TrustRegion.min_linf_distance) in float64 on the CPU; `dtype=torch.float32`
gives the fp32 torch emulation (CPU self-check), `device='cuda'` the code the
kernels replace (the measured margin of the GPU tests).

Shared by tests/test_setpe_cases.py (CPU) and tests/test_setpe_kernels.py
(GPU).
"""

import dataclasses
import functools
import math
from typing import Optional

import numpy as np
import torch

import qei_cases as qc
import scorer_cases as sc

U32 = 2.0 ** -24
JITTER = 1e-10 * sc.AMP2          # as the designer: 1e-10 * amp^2
EXPLORE_COEF = 0.5                # UCBPEConfig defaults
PENALTY_COEF = 10.0
LAMBDA_MIN = 5e-3                 # condition on every dense reference set

# (B, q, N, P, D), the smallest that cross each boundary: q = 1 / odd N /
# D = 1; N + P equal to the wave size; the q = 8, B = 25 sweep shape with
# N + P just past the 256-row reduction stride of the k-vector kernel (B q =
# 200 > 32 candidates: the explore posterior takes the legacy quadform, the
# first two shapes the 64 x 64 tile one); the q = 16 limit with B > 32 and a
# last workgroup that is not full; several strides of rows.
DENSE_SHAPES = [(1, 1, 63, 0, 1), (3, 2, 63, 1, 3), (25, 8, 255, 2, 20),
                (33, 16, 300, 5, 7), (5, 3, 1000, 0, 10)]
# A shape whose default seed breaks a condition gets another seed here.
SEEDS = {}


@dataclasses.dataclass
class Case:
  b: int
  q: int
  n: int
  p: int
  d: int
  explore: qc.Case       # completed-trials GP over x (n rows)
  var: qc.Case           # completed + pending GP over x_all, alpha = 0
  threshold: float       # fp32-representable

  @property
  def xs(self):
    return self.explore.xs


@dataclasses.dataclass
class Ref:
  scores: torch.Tensor       # (b,)
  logdet: torch.Tensor       # (b,) -inf where info != 0
  penalty: torch.Tensor      # (b,)
  tr: torch.Tensor           # (b,) 0 without a trust region
  cov: torch.Tensor          # (b, q, q) un-jittered
  info: torch.Tensor         # (b,)
  explore_ucb: torch.Tensor  # (b, q)
  dist: torch.Tensor         # (b, q) to x_all, unmasked unless a region is given


def make_case(b: int, q: int, n: int, p: int, d: int, seed: int = 0) -> Case:
  g = torch.Generator().manual_seed(seed)

  def r(*shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64)
  x = r(n, d).float()
  pending = r(p, d).float()
  xs = r(b, q, d).float()
  ls = (math.sqrt(d) * (0.3 + 0.3 * r(d))).float()
  alpha, kinv = qc.gp_operands(x, ls, g)
  if p:
    x_all = torch.cat([x, pending], dim=0)
    _, kinv_all = qc.gp_operands(x_all, ls, g)
  else:
    x_all, kinv_all = x, kinv
  eps = torch.zeros(1, q)
  explore = qc.Case(b, q, n, d, x, xs, ls, alpha, kinv, eps, 0.0)
  var = qc.Case(b, q, n + p, d, x_all, xs, ls, torch.zeros(n + p), kinv_all,
                eps, 0.0)
  case = Case(b, q, n, p, d, explore, var, 0.0)
  case.threshold = float(np.float32(reference(case).explore_ucb.median()))
  return case


@functools.lru_cache(maxsize=None)
def dense_case(b: int, q: int, n: int, p: int, d: int) -> Case:
  """The (shared, never mutated) dense case of a shape."""
  shape = (b, q, n, p, d)
  seed = SEEDS.get(shape, 100000 * q + 1000 * b + n + 7 * d + 31 * p)
  return make_case(*shape, seed=seed)


def trust_region(case: Case, radius: float, onehot=None,
                 dtype=torch.float64, device='cpu',
                 x_all: Optional[torch.Tensor] = None):
  """Production TrustRegion over x_all (or the given tensor of its rows),
  radius pinned."""
  from vizier_amd._src.gp import acquisitions as acq_lib
  if x_all is None:
    x_all = case.var.x.to(device=device, dtype=dtype)
  mask = torch.tensor(onehot if onehot is not None else [0] * case.d,
                      dtype=torch.bool, device=device)
  tr = acq_lib.TrustRegion(x_all, mask)
  tr.trust_radius = radius
  return tr


def tail_reference(cov, mean, sd, dist, jitter, threshold, explore_coef,
                   penalty_coef, tr_radius):
  """The score_fn body of _set_pe_score_fn after the posteriors, in the
  dtype and on the device of `cov`: (scores, logdet, penalty, tr, info).
  mean / sd / dist are (B, q); dist None means no trust region."""
  q = cov.shape[-1]
  explore_ucb = mean + explore_coef * sd
  penalty = penalty_coef * torch.minimum(
      explore_ucb - threshold, torch.zeros_like(explore_ucb)).sum(-1)
  eye = torch.eye(q, dtype=cov.dtype, device=cov.device)
  L, info = torch.linalg.cholesky_ex(cov + jitter * eye)
  logdet = 2.0 * torch.log(
      torch.diagonal(L, dim1=-2, dim2=-1).clamp_min(1e-30)).sum(-1)
  logdet = torch.where(info == 0, logdet,
                       torch.full_like(logdet, -float('inf')))
  scores = logdet + penalty
  tr = torch.zeros_like(scores)
  if dist is not None and tr_radius <= 0.5:
    tr = torch.where(dist > tr_radius, -1e4 - dist,
                     torch.zeros_like(dist)).sum(-1)
    scores = scores + tr
  return scores, logdet, penalty, tr, info


def reference(case: Case, dtype=torch.float64, device='cpu',
              region=None) -> Ref:
  """_set_pe_score_fn's torch closure in `dtype` on `device`."""
  from vizier_amd._src.algorithms.designers.gp_bandit import (
      posterior_batched_cov,
  )
  post = case.explore.posterior(dtype, device)
  var_post = case.var.posterior(dtype, device)
  xs = case.xs.to(device=device, dtype=dtype)
  flat = xs.reshape(case.b * case.q, -1)
  mean, sd = post.predict(flat)
  mean, sd = mean.reshape(case.b, case.q), sd.reshape(case.b, case.q)
  _, cov = posterior_batched_cov(var_post, xs)
  if region is not None:
    dist, radius = region.min_linf_distance(xs), region.trust_radius
  else:
    dist, radius = None, 0.0
  amp2 = float(var_post.params.amplitude) ** 2
  scores, logdet, penalty, tr, info = tail_reference(
      cov, mean, sd, dist, 1e-10 * amp2, case.threshold, EXPLORE_COEF,
      PENALTY_COEF, radius)
  if dist is None:
    dist = (flat[:, None, :] - var_post.x[None, :, :]).abs().amax(-1).amin(
        -1).reshape(case.b, case.q)
  return Ref(scores=scores, logdet=logdet, penalty=penalty, tr=tr, cov=cov,
             info=info, explore_ucb=mean + EXPLORE_COEF * sd, dist=dist)


@functools.lru_cache(maxsize=None)
def dense_reference(b: int, q: int, n: int, p: int, d: int) -> Ref:
  return reference(dense_case(b, q, n, p, d))


def score_floor(q: int, scores: torch.Tensor) -> torch.Tensor:
  """16 q u max(1, |score_ref|) per set: a q x q fp32 factorisation and
  q-term fp32 sums, each held to 16 roundings per term."""
  return 16.0 * q * U32 * scores.abs().clamp_min(1.0)


def split_radius(dist: torch.Tensor) -> float:
  """A radius in the widest gap between consecutive sorted distances of the
  middle half, so that about half the members are outside and none sits
  within rounding of the radius. fp32-representable."""
  flat = dist.flatten().sort().values
  lo, hi = len(flat) // 4, max(len(flat) // 4 + 1, 3 * len(flat) // 4)
  gaps = flat[lo + 1:hi + 1] - flat[lo:hi]
  i = int(gaps.argmax()) + lo
  return float(np.float32(0.5 * (flat[i] + flat[i + 1])))


def logdet_bound(case: Case, ref: Ref) -> torch.Tensor:
  """(b,) first-order bound on the logdet error of an fp32 evaluation:
  d logdet(A) = tr(A^-1 dA) <= sum_rc |A^-1|_rc |dA|_rc, with |dA| the
  per-entry covariance bound of qei_cases.joint_bounds (fp32 accumulation of
  the two chained N-term sums and the k-vector rounding) plus one rounding
  of the jittered diagonal, doubled for the higher-order terms, plus the
  q 2^-22 max(1, max|log pivot|) of the factorisation itself."""
  jref = qc.joint_reference(case.var)
  _, cov_bound = qc.joint_bounds(case.var, jref)
  eye = torch.eye(case.q, dtype=torch.float64)
  a = ref.cov + JITTER * eye
  cov_bound = cov_bound + 2.0 * U32 * a.abs()
  inv = torch.linalg.inv(a).abs()
  piv = torch.linalg.cholesky(a).diagonal(dim1=-2, dim2=-1) ** 2
  fact = case.q * 2.0 ** -22 * piv.log().abs().amax(-1).clamp_min(1.0)
  return 2.0 * (inv * cov_bound).sum((-2, -1)) + fact


# -- hand-made tail inputs --------------------------------------------------


@dataclasses.dataclass
class Tail:
  """Inputs of the tail with the closed-form fp64 value of each set."""
  name: str
  cov: torch.Tensor              # (B, q, q) fp32
  mean: torch.Tensor             # (B, q) fp32
  sd: torch.Tensor               # (B, q) fp32
  dist: Optional[torch.Tensor]   # (B, q) fp32 or None
  threshold: float
  explore_coef: float
  penalty_coef: float
  tr_radius: float
  want: torch.Tensor             # (B,) fp64
  bound: torch.Tensor            # (B,) fp64

  def args(self, device):
    """Arguments of ext.setpe_scores_from_cov (jitter 0)."""
    dist = None if self.dist is None else self.dist.to(device)
    return (self.cov.to(device), self.mean.to(device), self.sd.to(device),
            dist, 0.0, self.threshold, self.explore_coef, self.penalty_coef,
            self.tr_radius)


def _tail(name, cov, log_pivots, mean=None, sd=None, dist=None,
          threshold=0.0, explore_coef=0.5, penalty_coef=10.0, tr_radius=0.0):
  """log_pivots: (B, q) fp64 closed-form log of every pivot. The penalty
  and trust-region sums are evaluated in fp64 from the fp32 inputs.

  Bound: q 2^-22 (max(1, max|log pivot|) + sum|penalty terms| +
  sum|trust-region terms|): every one of the three sums has q terms, each
  within an ulp or two of its value, and the final additions round at the
  magnitude of the largest of them."""
  b, q = cov.shape[0], cov.shape[-1]
  mean = torch.zeros(b, q) if mean is None else mean
  sd = torch.zeros(b, q) if sd is None else sd
  pen = penalty_coef * (mean.double() + explore_coef * sd.double() -
                        threshold).clamp_max(0.0)
  trt = torch.zeros(b, q, dtype=torch.float64)
  if dist is not None and 0.0 < tr_radius <= 0.5:
    # fp32 code compares with the radius rounded to fp32, so that a member
    # at float32(0.3) sits ON the radius 0.3: inside.
    dd = dist.double()
    trt = torch.where(dd > float(np.float32(tr_radius)), -1e4 - dd,
                      torch.zeros_like(dd))
  want = log_pivots.sum(-1) + pen.sum(-1) + trt.sum(-1)
  bound = q * 2.0 ** -22 * (log_pivots.abs().amax(-1).clamp_min(1.0) +
                            pen.abs().sum(-1) + trt.abs().sum(-1))
  return Tail(name, cov, mean, sd, dist, threshold, explore_coef,
              penalty_coef, tr_radius, want, bound)


def _diag_covs(q: int, seed: int):
  """(3, q, q) diagonal covariances, entries in [1e-3, 10] (log-uniform)."""
  g = torch.Generator().manual_seed(seed)
  diag = torch.exp(math.log(1e-3) + math.log(1e4) * torch.rand(
      3, q, generator=g, dtype=torch.float64)).float()
  return torch.diag_embed(diag), diag.double().log()


def handmade_tails():
  tails = []
  for q in (1, 2, 16):
    cov, logs = _diag_covs(q, seed=q)
    tails.append(_tail(f'diagonal q={q}', cov, logs))
  # 2 x 2 [[a, b], [b, c]]: logdet = log(a c - b^2); pivots a and c - b^2/a.
  abc = torch.tensor([[2.0, 0.5, 1.0], [1.0, -0.25, 0.5], [4.0, 1.0, 3.0]])
  a, b_, c = (abc[:, i].double() for i in range(3))
  cov2 = torch.stack([torch.stack([abc[:, 0], abc[:, 1]], -1),
                      torch.stack([abc[:, 1], abc[:, 2]], -1)], -2)
  logs2 = torch.stack([a.log(), (c - b_ * b_ / a).log()], -1)
  assert torch.allclose(logs2.sum(-1), (a * c - b_ * b_).log(), rtol=0,
                        atol=1e-14)
  tails.append(_tail('2x2', cov2, logs2))
  # Penalty: no / some / all members below the threshold (q = 4, cov = I).
  eye4 = torch.eye(4).expand(3, 4, 4).contiguous()
  zero4 = torch.zeros(3, 4, dtype=torch.float64)
  mean = torch.tensor([[0.9, 1.2, 0.8, 2.0], [0.9, -0.3, 0.8, 0.1],
                       [-1.0, -0.3, 0.2, 0.1]])
  sd = torch.tensor([[0.1, 0.2, 0.3, 0.4]]).expand(3, 4).contiguous()
  tails.append(_tail('penalty', eye4, zero4, mean=mean, sd=sd,
                     threshold=0.75))
  # Trust region: 0, 1 and all members outside radius 0.3.
  dist = torch.tensor([[0.1, 0.2, 0.25, 0.3], [0.1, 0.45, 0.25, 0.3],
                       [0.31, 0.45, 0.9, 0.5]])
  tails.append(_tail('trust region', eye4, zero4, dist=dist, tr_radius=0.3))
  # Radius 0.6 (> 0.5: the region is off) and dist = None.
  tails.append(_tail('trust region off', eye4, zero4, dist=dist,
                     tr_radius=0.6))
  tails.append(_tail('no trust region', eye4, zero4, dist=None,
                     tr_radius=0.3))
  # Everything at once.
  tails.append(_tail('all terms', cov2, logs2, mean=mean[:, :2],
                     sd=sd[:, :2], dist=dist[:, :2], threshold=0.75,
                     tr_radius=0.3))
  return tails


NAN = float('nan')
BAD_COVS = [[[1.0, 2.0], [2.0, 1.0]],           # indefinite
            [[0.0, 0.0], [0.0, 0.0]],           # zero
            [[0.5, NAN], [NAN, 2.0]],           # NaN off-diagonals
            [[NAN, 0.0], [0.0, 1.0]]]           # NaN first pivot
GOOD_COVS = [[[1.0, 0.3], [0.3, 0.5]], [[2.0, -1.0], [-1.0, 1.5]],
             [[0.2, 0.0], [0.0, 0.1]]]
