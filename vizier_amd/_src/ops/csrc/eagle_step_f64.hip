// fp64 Eagle-strategy suggest/update kernels for gfx950 (parity mode).
//
// A port of eagle_step.hip with the pool, rewards, perturbations, outputs
// and best_reward in `double`: same one-workgroup-per-firefly shape, same
// MAX_POOL / MAX_Q, same two-slot device iteration counter handshake, so
// the fp64 sweep is captured in a hipGraph exactly like the fp32 one.
//
// RNG: the same integers as the fp32 kernels for the same
// (seed, offset, idx) (vz_splitmix64); the 24-bit uniform is widened
// exactly, Laplace / Gumbel / the force use log1p, log and exp in double
// (common_f64.h). The stream therefore differs from the torch fp64 path.
//
// Algorithm spec: vizier_amd/_src/algorithms/optimizers/eagle.py.

#include <hip/hip_runtime.h>
#include "common_f64.h"

#define BLOCK 256
#define MAX_POOL 128
#define MAX_Q 16

// -- suggest -----------------------------------------------------------------

extern "C" __global__ __launch_bounds__(BLOCK) void
eagle_suggest_f64_kernel(
    const double* __restrict__ pool_cont,      // (P, q, Dc)
    const long* __restrict__ pool_cat,         // (P, q, Dcat)
    const double* __restrict__ rewards,        // (P,)
    const double* __restrict__ perturbations,  // (P,)
    const long* __restrict__ cat_sizes,        // (Dcat,)
    double* __restrict__ out_cont,             // (B, q, Dc)
    long* __restrict__ out_cat,                // (B, q, Dcat)
    const unsigned long long* __restrict__ iter_ptr, int n_batches,
    int batch_size, int pool_size, int q, int dc, int dcat, int max_cat,
    double visibility, double gravity, double neg_gravity,
    double norm_scale, double cat_factor, double p_same,
    unsigned long long seed) {
  // Counter handshake, as in eagle_suggest_kernel: suggest reads slot 0
  // and publishes the iteration to slot 1 for the update kernel; update
  // reads slot 1 and advances slot 0. Ordering comes from the stream.
  const unsigned long long offset = iter_ptr[0];
  const int batch_start = (int)(offset % (unsigned long long)n_batches) *
                          batch_size;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ((unsigned long long*)iter_ptr)[1] = offset;
  }
  __shared__ double scale[MAX_POOL];
  __shared__ double red[8];
  __shared__ double scale_sum_s;

  const int b = blockIdx.x;
  if (b >= batch_size) return;
  const int me = batch_start + b;      // pool index of this firefly
  const int tid = threadIdx.x;
  const int n_features = dc + dcat;
  const int flat_c = q * dc;
  const double my_reward = rewards[me];
  const double my_pert = perturbations[me];

  // Phase 1: per-pool-member force -> scale[p].
  for (int p = tid; p < pool_size; p += BLOCK) {
    double d2 = 0.0;
    for (int j = 0; j < flat_c; ++j) {
      const double diff = pool_cont[me * flat_c + j] -
                          pool_cont[p * flat_c + j];
      d2 = fma(diff, diff, d2);
    }
    for (int j = 0; j < q * dcat; ++j) {
      d2 += (pool_cat[me * q * dcat + j] != pool_cat[p * q * dcat + j])
                ? 1.0 : 0.0;
    }
    const double reward_p = rewards[p];
    const double dir = (reward_p - my_reward >= 0.0) ? gravity
                                                     : -neg_gravity;
    const double force = exp(-visibility * d2 / n_features * 10.0);
    double s = dir * force;
    if (!isfinite(reward_p)) s = 0.0;
    scale[p] = s;
  }
  __syncthreads();

  // Counts for MEAN normalization.
  double pulls = 0.0, pushes = 0.0;
  for (int p = tid; p < pool_size; p += BLOCK) {
    pulls += (scale[p] > 0.0) ? 1.0 : 0.0;
    pushes += (scale[p] < 0.0) ? 1.0 : 0.0;
  }
  auto dsum = [](double a, double c) { return a + c; };
  const double n_pull = block_reduce_f64(pulls, red, dsum, 0.0);
  if (tid == 0) red[4] = fmax(n_pull, 1.0);
  __syncthreads();
  const double n_push = block_reduce_f64(pushes, red, dsum, 0.0);
  if (tid == 0) red[5] = fmax(n_push, 1.0);
  __syncthreads();
  const double inv_pull = 1.0 / red[4];
  const double inv_push = 1.0 / red[5];

  // Normalize scale in place; accumulate its sum.
  double ssum = 0.0;
  for (int p = tid; p < pool_size; p += BLOCK) {
    const double s = scale[p];
    const double ns = norm_scale * (s > 0.0 ? s * inv_pull : s * inv_push);
    scale[p] = ns;
    ssum += ns;
  }
  __syncthreads();
  double scale_sum = block_reduce_f64(ssum, red, dsum, 0.0);
  if (tid == 0) scale_sum_s = scale_sum;
  __syncthreads();
  scale_sum = scale_sum_s;

  // Phase 2: continuous move + laplace perturbation. Threads over dims.
  for (int j = tid; j < flat_c; j += BLOCK) {
    double moved = 0.0;
    for (int p = 0; p < pool_size; ++p) {
      moved = fma(scale[p], pool_cont[p * flat_c + j], moved);
    }
    const double mine = pool_cont[me * flat_c + j];
    moved = mine + (moved - mine * scale_sum);
    // Laplace noise normalized over the q axis for this (b, dim).
    const int dim = j % dc;
    double noise = vz_rng_laplace_f64(seed, offset,
                                      (unsigned)(b * flat_c + j));
    if (q > 1) {
      double maxabs = 1e-12;
      for (int qq = 0; qq < q; ++qq) {
        const double nv = vz_rng_laplace_f64(
            seed, offset, (unsigned)(b * flat_c + qq * dc + dim));
        maxabs = fmax(maxabs, fabs(nv));
      }
      noise /= maxabs;
    } else {
      noise = (noise >= 0.0) ? 1.0 : -1.0;  // |laplace|/max == 1
    }
    out_cont[b * flat_c + j] = moved + noise * my_pert;
  }

  // Phase 3: categorical mutation. Threads over (q, dcat) pairs.
  for (int jd = tid; jd < q * dcat; jd += BLOCK) {
    const int dimc = jd % dcat;
    const long size = cat_sizes[dimc];
    const double logit_same = log(p_same);
    const double logit_diff = log((1.0 - p_same) /
                                  fmax((double)size - 1.0, 1e-9));
    const long cur = pool_cat[me * q * dcat + jd];
    const double pert_noise =
        vz_rng_laplace_f64(seed, offset ^ 0x9e01ull,
                           (unsigned)(b * q * dcat + jd)) *
        cat_factor * my_pert;
    double best_val = -INFINITY;
    long best_cat = cur;
    for (long c = 0; c < size; ++c) {
      double ssum_c = 0.0;
      for (int p = 0; p < pool_size; ++p) {
        if (pool_cat[p * q * dcat + jd] == c) ssum_c += scale[p];
      }
      // logits[c] = sum_p scale[p][cat_p == c] + logit_diff, and at the
      // current category: + (-sum(scale) + logit_same - logit_diff).
      double logit = ssum_c + logit_diff;
      if (c == cur) logit += -scale_sum_s + logit_same - logit_diff;
      logit += pert_noise;
      // Gumbel-max sampling.
      const double u = vz_rng_uniform_f64(
          seed, offset ^ 0x77aaull,
          (unsigned)((b * q * dcat + jd) * max_cat + (int)c));
      const double g = -log(-log(fmax(u, 1e-20)));
      if (logit + g > best_val) {
        best_val = logit + g;
        best_cat = c;
      }
    }
    out_cat[b * q * dcat + jd] = best_cat;
  }
}

// -- update ------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(BLOCK) void
eagle_update_f64_kernel(double* __restrict__ pool_cont,
                        long* __restrict__ pool_cat,
                        double* __restrict__ rewards,
                        double* __restrict__ perturbations,
                        const double* __restrict__ batch_cont,
                        const long* __restrict__ batch_cat,
                        const double* __restrict__ batch_rewards,
                        const long* __restrict__ cat_sizes,
                        double* __restrict__ best_reward,
                        unsigned long long* __restrict__ iter_ptr,
                        int n_batches, int batch_size, int q, int dc,
                        int dcat, double penalize_factor,
                        double perturbation_lower_bound,
                        double base_perturbation,
                        unsigned long long seed) {
  // One block per batch member. Every block recomputes the (tiny) batch
  // max + old best, so new_best is identical everywhere and writes are
  // idempotent: no cross-block ordering needed.
  const unsigned long long offset = iter_ptr[1];
  const int batch_start = (int)(offset % (unsigned long long)n_batches) *
                          batch_size;
  __shared__ double red[8];
  __shared__ double new_best_s;
  const int tid = threadIdx.x;
  const int i = blockIdx.x;
  if (i >= batch_size) return;

  double local_max = -INFINITY;
  for (int t = tid; t < batch_size; t += BLOCK) {
    local_max = fmax(local_max, batch_rewards[t]);
  }
  auto dmax = [](double a, double c) { return fmax(a, c); };
  const double batch_max = block_reduce_f64(local_max, red, dmax,
                                            -(double)INFINITY);
  if (tid == 0) {
    new_best_s = fmax(best_reward[0], batch_max);
    if (i == 0) best_reward[0] = new_best_s;
  }
  __syncthreads();
  const double new_best = new_best_s;
  const int flat_c = q * dc;
  const int flat_k = q * dcat;

  const int me = batch_start + i;
  const double new_r = batch_rewards[i];
  const double old_r = rewards[me];
  const bool improved = new_r > old_r;
  double pert = improved ? perturbations[me]
                         : perturbations[me] * penalize_factor;
  double reward = improved ? new_r : old_r;
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
      pool_cont[me * flat_c + j] = vz_rng_uniform_f64(
          seed, offset ^ 0x5151ull, (unsigned)(me * flat_c + j));
    }
    for (int j = tid; j < flat_k; j += BLOCK) {
      const long size = cat_sizes[j % dcat];
      const double u = vz_rng_uniform_f64(seed, offset ^ 0x1234ull,
                                          (unsigned)(me * flat_k + j));
      long c = (long)(u * (double)size);
      pool_cat[me * flat_k + j] = min(c, size - 1);
    }
    reward = -INFINITY;
    pert = base_perturbation;
  }
  if (tid == 0) {
    rewards[me] = reward;
    perturbations[me] = pert;
    if (i == 0) iter_ptr[0] = offset + 1;  // next suggest's iteration
  }
}

// -- launchers ---------------------------------------------------------------

extern "C" void launch_eagle_suggest_f64(
    const double* pool_cont, const long* pool_cat, const double* rewards,
    const double* perturbations, const long* cat_sizes, double* out_cont,
    long* out_cat, const unsigned long long* iter_ptr, int n_batches,
    int batch_size, int pool_size, int q, int dc, int dcat, int max_cat,
    double visibility, double gravity, double neg_gravity,
    double norm_scale, double cat_factor, double p_same,
    unsigned long long seed, hipStream_t stream) {
  hipLaunchKernelGGL(eagle_suggest_f64_kernel, dim3(batch_size),
                     dim3(BLOCK), 0, stream, pool_cont, pool_cat, rewards,
                     perturbations, cat_sizes, out_cont, out_cat, iter_ptr,
                     n_batches, batch_size, pool_size, q, dc, dcat,
                     max_cat, visibility, gravity, neg_gravity, norm_scale,
                     cat_factor, p_same, seed);
}

extern "C" void launch_eagle_update_f64(
    double* pool_cont, long* pool_cat, double* rewards,
    double* perturbations, const double* batch_cont, const long* batch_cat,
    const double* batch_rewards, const long* cat_sizes,
    double* best_reward, unsigned long long* iter_ptr, int n_batches,
    int batch_size, int q, int dc, int dcat, double penalize_factor,
    double perturbation_lower_bound, double base_perturbation,
    unsigned long long seed, hipStream_t stream) {
  hipLaunchKernelGGL(eagle_update_f64_kernel, dim3(batch_size),
                     dim3(BLOCK), 0, stream, pool_cont, pool_cat, rewards,
                     perturbations, batch_cont, batch_cat, batch_rewards,
                     cat_sizes, best_reward, iter_ptr, n_batches,
                     batch_size, q, dc, dcat, penalize_factor,
                     perturbation_lower_bound, base_perturbation, seed);
}
