// Fused Eagle-strategy suggest/update kernels for gfx950.
//
// One workgroup per batch firefly. Replaces ~30 eager tensor launches
// per Eagle iteration with two: suggest (distances -> forces -> moves ->
// perturbation + categorical sampling) and update (accept/penalize/trim).
// The pool (<= 100 flies x D features) is small enough that all inputs
// sit in L2; the kernels are launch-latency-bound by design, which is
// exactly what fusing minimizes.
//
// Both kernels are templates over the pool's precision T: float in
// production, double for the float64 parity mode, captured in a hipGraph
// the same way. Both draw the same RNG integers for the same (seed, offset,
// idx); Laplace / Gumbel / the force go through vz_math<T> (fast
// intrinsics in float, accurate libm in double).
//
// Algorithm spec: vizier_amd/_src/algorithms/optimizers/eagle.py (the
// torch implementation is the CPU oracle; RNG streams differ).

#include <hip/hip_runtime.h>
#include "common.h"

#define BLOCK 256
#define MAX_POOL 128
#define MAX_Q 16

// -- suggest -----------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(BLOCK) void
eagle_suggest_kernel(const T* __restrict__ pool_cont,      // (P, q, Dc)
                     const long* __restrict__ pool_cat,    // (P, q, Dcat)
                     const T* __restrict__ rewards,        // (P,)
                     const T* __restrict__ perturbations,  // (P,)
                     const long* __restrict__ cat_sizes,   // (Dcat,)
                     T* __restrict__ out_cont,             // (B, q, Dc)
                     long* __restrict__ out_cat,           // (B, q, Dcat)
                     const unsigned long long* __restrict__ iter_ptr,
                     int n_batches, int batch_size, int pool_size, int q,
                     int dc, int dcat, int max_cat, T visibility, T gravity,
                     T neg_gravity, T norm_scale, T cat_factor, T p_same,
                     unsigned long long seed) {
  using M = vz_math<T>;
  // Counter handshake (hipGraph-capturable, race-free): suggest reads
  // slot 0 and publishes the iteration to slot 1 for the update kernel;
  // update reads slot 1 and advances slot 0 for the next suggest. All
  // cross-kernel ordering comes from stream order; within a kernel only
  // one block writes, and readers never read the slot their own grid
  // writes.
  const unsigned long long offset = iter_ptr[0];
  const int batch_start = (int)(offset % (unsigned long long)n_batches) *
                          batch_size;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ((unsigned long long*)iter_ptr)[1] = offset;
  }
  __shared__ T scale[MAX_POOL];
  __shared__ T red[8];
  __shared__ T scale_sum_s;

  const int b = blockIdx.x;
  if (b >= batch_size) return;
  const int me = batch_start + b;      // pool index of this firefly
  const int tid = threadIdx.x;
  const int n_features = dc + dcat;
  const int flat_c = q * dc;
  const T my_reward = rewards[me];
  const T my_pert = perturbations[me];

  // Phase 1: per-pool-member force -> scale[p].
  for (int p = tid; p < pool_size; p += BLOCK) {
    T d2 = T(0);
    for (int j = 0; j < flat_c; ++j) {
      const T diff = pool_cont[me * flat_c + j] - pool_cont[p * flat_c + j];
      d2 = M::fma(diff, diff, d2);
    }
    for (int j = 0; j < q * dcat; ++j) {
      d2 += (pool_cat[me * q * dcat + j] != pool_cat[p * q * dcat + j])
                ? T(1) : T(0);
    }
    const T reward_p = rewards[p];
    const T dir = (reward_p - my_reward >= T(0)) ? gravity : -neg_gravity;
    const T force = M::exp(-visibility * d2 / n_features * T(10));
    T s = dir * force;
    if (!isfinite(reward_p)) s = T(0);
    scale[p] = s;
  }
  __syncthreads();

  // Counts for MEAN normalization.
  T pulls = T(0), pushes = T(0);
  for (int p = tid; p < pool_size; p += BLOCK) {
    pulls += (scale[p] > T(0)) ? T(1) : T(0);
    pushes += (scale[p] < T(0)) ? T(1) : T(0);
  }
  auto fsum = [](T a, T c) { return a + c; };
  T n_pull = block_reduce(pulls, red, fsum, T(0));
  if (tid == 0) red[4] = M::fmax(n_pull, T(1));
  __syncthreads();
  T n_push = block_reduce(pushes, red, fsum, T(0));
  if (tid == 0) red[5] = M::fmax(n_push, T(1));
  __syncthreads();
  const T inv_pull = T(1) / red[4];
  const T inv_push = T(1) / red[5];

  // Normalize scale in place; accumulate its sum.
  T ssum = T(0);
  for (int p = tid; p < pool_size; p += BLOCK) {
    const T s = scale[p];
    const T ns = norm_scale * (s > T(0) ? s * inv_pull : s * inv_push);
    scale[p] = ns;
    ssum += ns;
  }
  __syncthreads();
  T scale_sum = block_reduce(ssum, red, fsum, T(0));
  if (tid == 0) scale_sum_s = scale_sum;
  __syncthreads();
  scale_sum = scale_sum_s;

  // Phase 2: continuous move + laplace perturbation. Threads over dims.
  for (int j = tid; j < flat_c; j += BLOCK) {
    T moved = T(0);
    for (int p = 0; p < pool_size; ++p) {
      moved = M::fma(scale[p], pool_cont[p * flat_c + j], moved);
    }
    const T mine = pool_cont[me * flat_c + j];
    moved = mine + (moved - mine * scale_sum);
    // Laplace noise normalized over the q axis for this (b, dim).
    const int dim = j % dc;
    T noise = vz_rng_laplace<T>(seed, offset, (unsigned)(b * flat_c + j));
    if (q > 1) {
      T maxabs = T(1e-12);
      for (int qq = 0; qq < q; ++qq) {
        const T nv = vz_rng_laplace<T>(
            seed, offset, (unsigned)(b * flat_c + qq * dc + dim));
        maxabs = M::fmax(maxabs, M::fabs(nv));
      }
      noise /= maxabs;
    } else {
      noise = (noise >= T(0)) ? T(1) : T(-1);  // |laplace|/max == 1
    }
    out_cont[b * flat_c + j] = moved + noise * my_pert;
  }

  // Phase 3: categorical mutation. Threads over (q, dcat) pairs.
  for (int jd = tid; jd < q * dcat; jd += BLOCK) {
    const int dimc = jd % dcat;
    const long size = cat_sizes[dimc];
    const T logit_same = M::log(p_same);
    const T logit_diff = M::log((T(1) - p_same) /
                                M::fmax(T(size) - T(1), T(1e-9)));
    const long cur = pool_cat[me * q * dcat + jd];
    const T pert_noise =
        vz_rng_laplace<T>(seed, offset ^ 0x9e01ull,
                          (unsigned)(b * q * dcat + jd)) *
        cat_factor * my_pert;
    T best_val = -T(INFINITY);
    long best_cat = cur;
    for (long c = 0; c < size; ++c) {
      T ssum_c = T(0);
      for (int p = 0; p < pool_size; ++p) {
        if (pool_cat[p * q * dcat + jd] == c) ssum_c += scale[p];
      }
      // logits[c] = sum_p scale[p][cat_p == c] + logit_diff, and at the
      // current category: + (-sum(scale) + logit_same - logit_diff).
      T logit = ssum_c + logit_diff;
      if (c == cur) logit += -scale_sum_s + logit_same - logit_diff;
      logit += pert_noise;
      // Gumbel-max sampling.
      const T u = vz_rng_uniform<T>(
          seed, offset ^ 0x77aaull,
          (unsigned)((b * q * dcat + jd) * max_cat + (int)c));
      const T g = -M::log(-M::log(M::fmax(u, T(1e-20))));
      if (logit + g > best_val) {
        best_val = logit + g;
        best_cat = c;
      }
    }
    out_cat[b * q * dcat + jd] = best_cat;
  }
}

// -- update ------------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(BLOCK) void
eagle_update_kernel(T* __restrict__ pool_cont,
                    long* __restrict__ pool_cat,
                    T* __restrict__ rewards,
                    T* __restrict__ perturbations,
                    const T* __restrict__ batch_cont,
                    const long* __restrict__ batch_cat,
                    const T* __restrict__ batch_rewards,
                    const long* __restrict__ cat_sizes,
                    T* __restrict__ best_reward,
                    unsigned long long* __restrict__ iter_ptr,
                    int n_batches, int batch_size, int q, int dc, int dcat,
                    T penalize_factor, T perturbation_lower_bound,
                    T base_perturbation, unsigned long long seed) {
  using M = vz_math<T>;
  // One block per batch member. Every block recomputes the (tiny)
  // batch max + old best, so new_best is identical everywhere and
  // writes are idempotent — no cross-block ordering needed.
  const unsigned long long offset = iter_ptr[1];
  const int batch_start = (int)(offset % (unsigned long long)n_batches) *
                          batch_size;
  __shared__ T red[8];
  __shared__ T new_best_s;
  const int tid = threadIdx.x;
  const int i = blockIdx.x;
  if (i >= batch_size) return;

  T local_max = -T(INFINITY);
  for (int t = tid; t < batch_size; t += BLOCK) {
    local_max = M::fmax(local_max, batch_rewards[t]);
  }
  auto fmax_ = [](T a, T c) { return M::fmax(a, c); };
  T batch_max = block_reduce(local_max, red, fmax_, -T(INFINITY));
  if (tid == 0) {
    new_best_s = M::fmax(best_reward[0], batch_max);
    if (i == 0) best_reward[0] = new_best_s;
  }
  __syncthreads();
  const T new_best = new_best_s;
  const int flat_c = q * dc;
  const int flat_k = q * dcat;

  const int me = batch_start + i;
  const T new_r = batch_rewards[i];
  const T old_r = rewards[me];
  const bool improved = new_r > old_r;
  T pert = improved ? perturbations[me]
                    : perturbations[me] * penalize_factor;
  T reward = improved ? new_r : old_r;
  const bool dead = (pert < perturbation_lower_bound) &&
                    (reward != new_best);
  if (improved) {
    for (int j = tid; j < flat_c; j += BLOCK) {
      pool_cont[me * flat_c + j] = batch_cont[i * flat_c + j];
    }
    for (int j = tid; j < flat_k; j += BLOCK) {
      pool_cat[me * flat_k + j] = batch_cat[i * flat_k + j];
    }
  }
  if (dead) {
    for (int j = tid; j < flat_c; j += BLOCK) {
      pool_cont[me * flat_c + j] = vz_rng_uniform<T>(
          seed, offset ^ 0x5151ull, (unsigned)(me * flat_c + j));
    }
    for (int j = tid; j < flat_k; j += BLOCK) {
      const long size = cat_sizes[j % dcat];
      const T u = vz_rng_uniform<T>(seed, offset ^ 0x1234ull,
                                    (unsigned)(me * flat_k + j));
      long c = (long)(u * T(size));
      pool_cat[me * flat_k + j] = min(c, size - 1);
    }
    reward = -T(INFINITY);
    pert = base_perturbation;
  }
  if (tid == 0) {
    rewards[me] = reward;
    perturbations[me] = pert;
    if (i == 0) iter_ptr[0] = offset + 1;  // next suggest's iteration
  }
}

// -- launchers ---------------------------------------------------------------

// launch_eagle_suggest[_f64] and launch_eagle_update[_f64]: the same two
// launchers for each precision.
#define EAGLE_STEP_LAUNCHERS(T, SUFFIX)                                      \
  extern "C" void launch_eagle_suggest##SUFFIX(                              \
      const T* pool_cont, const long* pool_cat, const T* rewards,            \
      const T* perturbations, const long* cat_sizes, T* out_cont,            \
      long* out_cat, const unsigned long long* iter_ptr, int n_batches,      \
      int batch_size, int pool_size, int q, int dc, int dcat, int max_cat,   \
      T visibility, T gravity, T neg_gravity, T norm_scale, T cat_factor,    \
      T p_same, unsigned long long seed, hipStream_t stream) {               \
    hipLaunchKernelGGL(                                                      \
        eagle_suggest_kernel<T>, dim3(batch_size), dim3(BLOCK), 0, stream,   \
        pool_cont, pool_cat, rewards, perturbations, cat_sizes, out_cont,    \
        out_cat, iter_ptr, n_batches, batch_size, pool_size, q, dc, dcat,    \
        max_cat, visibility, gravity, neg_gravity, norm_scale, cat_factor,   \
        p_same, seed);                                                       \
  }                                                                          \
  extern "C" void launch_eagle_update##SUFFIX(                               \
      T* pool_cont, long* pool_cat, T* rewards, T* perturbations,            \
      const T* batch_cont, const long* batch_cat, const T* batch_rewards,    \
      const long* cat_sizes, T* best_reward, unsigned long long* iter_ptr,   \
      int n_batches, int batch_size, int q, int dc, int dcat,                \
      T penalize_factor, T perturbation_lower_bound, T base_perturbation,    \
      unsigned long long seed, hipStream_t stream) {                         \
    hipLaunchKernelGGL(                                                      \
        eagle_update_kernel<T>, dim3(batch_size), dim3(BLOCK), 0, stream,    \
        pool_cont, pool_cat, rewards, perturbations, batch_cont, batch_cat,  \
        batch_rewards, cat_sizes, best_reward, iter_ptr, n_batches,          \
        batch_size, q, dc, dcat, penalize_factor, perturbation_lower_bound,  \
        base_perturbation, seed);                                            \
  }

EAGLE_STEP_LAUNCHERS(float, )
EAGLE_STEP_LAUNCHERS(double, _f64)
