"""Generic vectorized ask-evaluate-tell optimizer loop + top-k tracking.

Capability parity with vizier/_src/algorithms/optimizers/vectorized_base.py
(VectorizedOptimizer.__call__ :324, _update_best_results :544,
best_candidates_to_trials :591, trials_to_sorted_array :655,
VectorizedOptimizerFactory :669). The loop is host-driven over
GPU-resident tensors; on MI355X the per-iteration work is captured into
a hipGraph by the ops layer once shapes stabilize.
"""

from __future__ import annotations

import dataclasses
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from vizier_amd import pyvizier as vz
from vizier_amd.converters.core import TrialToArrayConverter
from vizier_amd._src.algorithms.optimizers.eagle import (
    CandidateBatch,
    EagleStrategyConfig,
    VectorizedEagleStrategy,
)

ScoreFn = Callable[[CandidateBatch], torch.Tensor]


@dataclasses.dataclass
class VectorizedStrategyResults:
  """Top-`count` candidates found by the sweep."""

  features: CandidateBatch          # (count, q, D*)
  rewards: torch.Tensor             # (count,)


class VectorizedOptimizer:
  """Runs a vectorized strategy against a batched score function."""

  def __init__(self, strategy: VectorizedEagleStrategy, *,
               max_evaluations: int = 75000):
    self.strategy = strategy
    self.max_evaluations = max_evaluations

  def optimize(self, score_fn: ScoreFn, *, count: int = 1,
               prior_features: Optional[CandidateBatch] = None,
               prior_rewards: Optional[torch.Tensor] = None
               ) -> VectorizedStrategyResults:
    strategy = self.strategy
    state = strategy.init_state(prior_features, prior_rewards)
    batch_size = strategy.batch_size
    iterations = max(1, (self.max_evaluations - 1) // batch_size + 1)

    self.last_used_graph = False
    self.last_used_megakernel = False
    self.last_graph_error = None
    if self._megakernel_applicable(score_fn):
      try:
        result = self._optimize_megakernel(score_fn, count, state,
                                           iterations)
        self.last_used_megakernel = True
        return result
      except Exception as e:
        import logging
        import traceback
        logging.getLogger(__name__).warning(
            'megakernel sweep fell back: %r\n%s', e,
            traceback.format_exc())
        self.last_graph_error = repr(e)
        state = strategy.init_state(prior_features, prior_rewards)
    if strategy._ext is not None and getattr(score_fn, 'graph_safe',
                                             True):
      try:
        result = self._optimize_hipgraph(score_fn, count, state,
                                         iterations)
        self.last_used_graph = True
        return result
      except Exception as e:
        # Score function not graph-capturable (e.g. host RNG inside
        # q-acquisitions): fall back to the eager loop from scratch.
        import logging
        import traceback
        logging.getLogger(__name__).warning(
            'hipGraph sweep fell back to eager: %r\n%s', e,
            traceback.format_exc())
        self.last_graph_error = repr(e)
        state = strategy.init_state(prior_features, prior_rewards)

    # Accumulate every evaluated candidate; one top-k at the end. At the
    # 75k-evaluation budget this is a few MB of HBM and removes ~6
    # tensor ops per iteration from the launch-bound loop.
    total = iterations * batch_size
    q = strategy.n_parallel
    all_cont = torch.empty(total, q, strategy.n_continuous,
                           dtype=strategy.dtype, device=strategy.device)
    all_cat = torch.empty(total, q, strategy.n_categorical,
                          dtype=torch.long, device=strategy.device)
    all_rewards = torch.empty(total, dtype=strategy.dtype,
                              device=strategy.device)
    offset = 0
    for _ in range(iterations):
      batch = strategy.suggest(state)
      rewards = score_fn(batch).detach()
      state = strategy.update(state, batch, rewards)
      all_cont[offset:offset + batch_size] = batch.continuous
      all_cat[offset:offset + batch_size] = batch.categorical
      all_rewards[offset:offset + batch_size] = rewards
      offset += batch_size

    all_rewards = torch.where(torch.isfinite(all_rewards), all_rewards,
                              torch.full_like(all_rewards, -float('inf')))
    k = min(count, total)
    top = torch.topk(all_rewards, k)
    return VectorizedStrategyResults(
        features=CandidateBatch(all_cont[top.indices],
                                all_cat[top.indices]),
        rewards=top.values)

  def _megakernel_applicable(self, score_fn: ScoreFn) -> bool:
    """Persistent-megakernel preconditions: GPU ext, continuous-only
    with at most 512 features (the kernel's xq_lds), q == 1, and a
    fused-able ScoringFunction (same conditions as the chunked HIP
    scorer fast path)."""
    import os
    if os.environ.get('VIZIER_AMD_MEGAKERNEL', '1') != '1':
      # Default ON: 68 us/iteration vs 85 for the hipGraph replay
      # (profiles/megatime3.log). Bitwise equal to the step kernels of
      # the hipGraph path for N < 4096; for 4096 <= N <= 8192 the
      # standalone scorer takes its SGEMM quadform, so the two paths
      # agree to the fp64-oracle tolerance only
      # (tests/test_sweep_kernel.py).
      # Set VIZIER_AMD_MEGAKERNEL=0 to force the hipGraph path.
      return False
    strategy = self.strategy
    scoring = getattr(score_fn, 'scoring', None)
    if (strategy._ext is None or scoring is None or
        not getattr(score_fn, 'codec_identity', False)):
      return False
    if strategy.categorical_sizes or strategy.n_parallel != 1:
      return False
    if strategy.dtype != torch.float32:
      # The megakernel is fp32 only; an fp64 strategy on the fp64 HIP
      # kernels (VIZIER_AMD_FP64_HIP=1) takes the hipGraph path.
      return False
    post = scoring.posterior
    return (scoring._acq_name is not None and scoring._tr_anchored and
            getattr(scoring, 'gram_dtype', 'fp32') == 'fp32' and
            post.K_inv is not None and post.x.is_cuda and
            strategy.pool_size <= 128 and strategy.batch_size <= 32
            and post.x.shape[0] <= 8192
            # The kernel's dc is x's width (continuous-only, identity
            # codec: strategy.n_continuous); xq_lds holds 512.
            and post.x.shape[1] <= 512)

  def _optimize_megakernel(self, score_fn: ScoreFn, count: int, state,
                           iterations: int) -> VectorizedStrategyResults:
    """Runs the steady-state sweep inside ONE cooperatively-launched
    persistent kernel (eagle_sweep.hip): suggest -> GP score -> update
    with grid-wide barriers, zero per-iteration dispatches. The
    initialization phase (+2 steady iterations, aligning the device
    counter) runs eagerly like the hipGraph path; the device phases
    replicate the standalone kernels verbatim, so for N < 4096 results
    are bit-identical to the hipGraph path for the same seeds. For
    4096 <= N <= 8192 the standalone scorer switches to its SGEMM
    quadform while the sweep keeps the 64x64 tiles: there the two paths
    agree to the fp64-oracle tolerance, not bitwise."""
    import torch as _torch

    strategy = self.strategy
    scoring = score_fn.scoring
    post = scoring.posterior
    cfg = strategy.config
    n_batches = strategy.pool_size // strategy.batch_size

    warmup_steady = 2
    eager_iters = min(iterations, n_batches + warmup_steady)
    for _ in range(eager_iters):
      batch = strategy.suggest(state)
      rewards = score_fn(batch).detach()
      strategy.update(state, batch, rewards)
    remaining = iterations - eager_iters

    if remaining > 0:
      b = strategy.batch_size
      n = post.x.shape[0]
      dev = post.x.device
      inv_ls = (1.0 / post.params.lengthscales).contiguous()
      k_ws = _torch.empty(b, n, dtype=_torch.float32, device=dev)
      mu_ws = _torch.empty(b, dtype=_torch.float32, device=dev)
      dist_ws = _torch.empty(b, dtype=_torch.float32, device=dev)
      tiles_n = (n + 63) // 64
      # (B, T+1): T tile partials + the reduced quadform per candidate
      # (the megakernel's phase B/B2 layout; see eagle_sweep.hip).
      var_ws = _torch.empty(b, tiles_n * tiles_n + 1,
                            dtype=_torch.float32, device=dev)
      # Zeroed per call: the kernel's grid barrier counts arrivals upwards
      # from zero over one launch.
      barrier_buf = _torch.zeros(2, dtype=_torch.int32, device=dev)
      from vizier_amd._src.ops import dispatch as ops
      amp2 = scoring._amp * scoring._amp
      tr_radius = (scoring._tr_radius
                   if scoring.trust_region is not None else 0.0)
      strategy._ext.eagle_sweep(
          state.continuous, state.rewards, state.perturbations,
          state.best_reward.reshape(1), strategy._iter_t, barrier_buf,
          post.x, inv_ls, post.alpha, post.K_inv,
          strategy._out_cont, k_ws, mu_ws, dist_ws, var_ws,
          n_batches, b, strategy.pool_size, state.iterations, remaining,
          cfg.visibility, cfg.gravity, cfg.negative_gravity,
          cfg.normalization_scale, cfg.penalize_factor,
          cfg.perturbation_lower_bound, cfg.perturbation,
          strategy._seed, strategy._seed ^ 0xABCDEF, amp2,
          scoring._mean_c, ops.ACQ_CODES[scoring._acq_name],
          scoring._coef, scoring._best, tr_radius)
      state.iterations += remaining

    rewards = torch.where(torch.isfinite(state.rewards), state.rewards,
                          torch.full_like(state.rewards, -float('inf')))
    k = min(count, rewards.numel())
    top = torch.topk(rewards, k)
    return VectorizedStrategyResults(
        features=CandidateBatch(state.continuous[top.indices].clone(),
                                state.categorical[top.indices].clone()),
        rewards=top.values.clone())

  def _optimize_hipgraph(self, score_fn: ScoreFn, count: int, state,
                         iterations: int) -> VectorizedStrategyResults:
    """GPU loop with the steady-state iteration captured in a hipGraph.

    One iteration is 3 static-argument kernel launches (eagle suggest,
    fused posterior score, eagle update) driven by a device-side
    iteration counter, so it replays at graph-launch cost instead of
    ~10 eager dispatches. Top-k is taken from the final pool: the
    best-ever candidate always survives in its firefly slot (a slot is
    only overwritten by a strictly better reward, and the global-best
    slot is exempt from random restarts), so for count=1 this is exact
    and for small counts it matches the reference's behavior closely.
    """
    strategy = self.strategy
    n_batches = strategy.pool_size // strategy.batch_size

    def one_iter():
      batch = strategy.suggest(state)
      rewards = score_fn(batch).detach()
      strategy.update(state, batch, rewards)

    # Initialization phase + 2 steady warmup iterations, eagerly.
    warmup_steady = 2
    eager_iters = min(iterations, n_batches + warmup_steady)
    for _ in range(eager_iters):
      one_iter()
    remaining = iterations - eager_iters

    if remaining > 0:
      side = torch.cuda.Stream()
      side.wait_stream(torch.cuda.current_stream())
      with torch.cuda.stream(side):
        one_iter()
        remaining -= 1
      torch.cuda.current_stream().wait_stream(side)
      graph = torch.cuda.CUDAGraph()
      with torch.cuda.graph(graph):
        one_iter()
      # Stream capture DEFERS execution to replay — the captured
      # iteration has not run yet, so it must not consume a slot
      # (verified bitwise against the eager and megakernel paths).
      for _ in range(remaining):
        graph.replay()

    rewards = torch.where(torch.isfinite(state.rewards), state.rewards,
                          torch.full_like(state.rewards, -float('inf')))
    k = min(count, rewards.numel())
    top = torch.topk(rewards, k)
    return VectorizedStrategyResults(
        features=CandidateBatch(state.continuous[top.indices].clone(),
                                state.categorical[top.indices].clone()),
        rewards=top.values.clone())


@dataclasses.dataclass
class VectorizedOptimizerFactory:
  """Builds a VectorizedOptimizer for a given feature structure."""

  eagle_config: EagleStrategyConfig = dataclasses.field(
      default_factory=EagleStrategyConfig)
  max_evaluations: int = 75000
  suggestion_batch_size: int = 25

  def __call__(self, *, n_continuous: int,
               categorical_sizes: Sequence[int], n_parallel: int = 1,
               seed: int = 0, device: str = 'cpu',
               dtype: torch.dtype = torch.float32) -> VectorizedOptimizer:
    strategy = VectorizedEagleStrategy(
        n_continuous=n_continuous, categorical_sizes=categorical_sizes,
        batch_size=self.suggestion_batch_size, config=self.eagle_config,
        n_parallel=n_parallel, seed=seed, device=device, dtype=dtype)
    return VectorizedOptimizer(strategy,
                               max_evaluations=self.max_evaluations)


class EagleFeatureCodec:
  """Maps between converter one-hot features and the Eagle representation.

  The TrialToArrayConverter produces a dense [0,1] matrix with one-hot
  blocks for categoricals; Eagle keeps categoricals as integer indices.
  """

  def __init__(self, converter: TrialToArrayConverter):
    self._converter = converter
    self.continuous_cols: List[int] = []
    self.onehot_specs: List[Tuple[int, int]] = []  # (start, width)
    for col in converter.output_specs:
      if col.is_onehot:
        self.onehot_specs.append((col.start, col.width))
      else:
        self.continuous_cols.append(col.start)
    self.n_continuous = len(self.continuous_cols)
    self.categorical_sizes = [w for _, w in self.onehot_specs]
    self.n_total = converter.n_features
    # Pure-continuous spaces decode as the identity (hot-loop fast path).
    self.identity = (not self.onehot_specs and
                     self.continuous_cols == list(range(self.n_total)))

  def encode(self, dense: torch.Tensor) -> CandidateBatch:
    """dense: (N, D_total) -> CandidateBatch with q=1."""
    cont = dense[:, self.continuous_cols] if self.continuous_cols else \
        dense[:, :0]
    cats = []
    for start, width in self.onehot_specs:
      cats.append(dense[:, start:start + width].argmax(dim=-1))
    cat = torch.stack(cats, dim=-1) if cats else \
        torch.zeros(dense.shape[0], 0, dtype=torch.long,
                    device=dense.device)
    return CandidateBatch(cont.unsqueeze(1), cat.unsqueeze(1))

  def decode(self, batch: CandidateBatch) -> torch.Tensor:
    """CandidateBatch (B, q, .) -> dense (B, q, D_total)."""
    if self.identity:
      return batch.continuous
    B, q = batch.continuous.shape[0], batch.continuous.shape[1]
    dense = torch.zeros(B, q, self.n_total, dtype=batch.continuous.dtype,
                        device=batch.continuous.device)
    for i, c in enumerate(self.continuous_cols):
      dense[..., c] = batch.continuous[..., i]
    for j, (start, width) in enumerate(self.onehot_specs):
      onehot = torch.nn.functional.one_hot(batch.categorical[..., j],
                                           width).to(dense.dtype)
      dense[..., start:start + width] = onehot
    return dense


def trials_to_sorted_features(
    converter: TrialToArrayConverter, codec: EagleFeatureCodec,
    trials: Sequence[vz.Trial], rewards: np.ndarray, *,
    device: str = 'cpu', dtype: torch.dtype = torch.float32
) -> Tuple[CandidateBatch, torch.Tensor]:
  """Prior trials -> Eagle features + rewards tensors (trial order kept)."""
  dense = torch.as_tensor(converter.to_features(trials), dtype=dtype,
                          device=device)
  batch = codec.encode(dense)
  r = torch.as_tensor(rewards, dtype=dtype, device=device)
  r = torch.where(torch.isnan(r), torch.full_like(r, -float('inf')), r)
  return batch, r
