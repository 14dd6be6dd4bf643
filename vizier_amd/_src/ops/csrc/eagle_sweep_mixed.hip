// Persistent Eagle-sweep megakernel for MIXED search spaces on gfx950:
// categorical + continuous parameters, or categorical ones alone.
//
// The variant of eagle_sweep_kernel (eagle_sweep.hip: read its header for
// the coherence design, the grid barrier and the parity scratch) that
// carries the categorical half of the Eagle state. Without it every study
// with one categorical parameter replays, per iteration, eagle_suggest,
// the codec's decode (one strided copy per continuous column, one_hot +
// cast + slice store per categorical parameter), the three scorer
// launches and eagle_update from a hipGraph.
//
// Scope: q == 1, fp32, RESIDENT mode only (pool_size * dc <= RESIDENT_CAP
// and pool_size * dcat <= RESIDENT_CAT_CAP), D = x.shape[1] <= 512 dense
// feature columns, N < 4096 in the optimizer (the binding takes up to
// 8192). There is no legacy form and no per-iteration pool staging; the
// barriers are the resident ones:
//   folded (N <= 2048)   A | B | RC          2 grid barriers
//   not folded           A | B | B2 | RC     3 grid barriers
// Phases B and B2, the reduce of RC, grid_sync and the block reductions
// are eagle_sweep_common.h's, the text eagle_sweep_kernel runs.
//
// State. Each owning workgroup (blockIdx.x < batch_size) keeps, for the
// whole launch, a private LDS copy of
//   the continuous pool        upper half of pool_lds, (P, dc) floats
//   the categorical pool       st_cat, (P, dcat) 16-bit indices (a
//                              category index is below D <= 512)
//   rewards / perturbations / best_reward
// and four parameter tables built once in the prologue: size, first
// (parameter, category) pair and first dense column of every categorical
// parameter, and the parameter of every pair. pool_cat stays int64 in
// global memory, as the strategy holds it; workgroup 0 writes both halves
// back after the last iteration.
//
// Phase A (owner of candidate b, half 0, the arithmetic of
// eagle_suggest_kernel at q == 1, same values from the same operations in
// the same order):
//   1. squared distance: the continuous fma chain, then + 1 per differing
//      categorical column, j = 0 .. dcat - 1; force over dc + dcat
//   2. pull / push counts, normalisation, scale_sum: as eagle_sweep_kernel
//   3. continuous move + sign noise: thread per column, written to the
//      dense column cont_cols[j] of xq_lds
//   4. categorical mutation. The step kernel gives one thread a whole
//      parameter, which walks size x pool entries serially; here that
//      would be the longest chain of the iteration. Instead thread e owns
//      the (parameter, category) PAIR e (at most D - dc <= 512 pairs, two
//      trips of 256): it sums scale[p] over p = 0 .. P - 1 where the
//      pool's category equals c (SG_PCHUNK LDS loads in flight; a
//      non-matching firefly leaves the sum as it is, so the sum has the
//      step kernel's bits), adds the logit terms, the Laplace
//      perturbation (offset ^ 0x9e01, drawn per pair: a hash and a log
//      cost less than a barrier to share them) and the Gumbel draw
//      (offset ^ 0x77aa, index (b dcat + j) max_cat + c), and leaves
//      logit + g in LDS. After ONE __syncthreads thread j scans its
//      parameter's pairs c = 0 .. size - 1 with a strict >, which picks
//      the lowest category among equal maxima as the step kernel's scan
//      does, and writes the choice to out_cat, the parity slot and, as a
//      one-hot block, to the dense columns cat_start[j] .. of xq_lds:
//      the layout EagleFeatureCodec.decode produces.
//   5. k-vector, mean and trust-region distance over the D dense columns
//      (sweep_kvec_mixed: sweep_kvec's loop plus the scorer's uint8
//      column mask; a masked column adds to d2 and not to the L-inf
//      distance).
// RC: eagle_update_kernel for all batch fireflies on the private copy. An
// improved firefly also takes the candidate's categories from the parity
// slot; a dead one redraws them as min((long)(u size), size - 1), u at
// offset ^ 0x1234, index me dcat + j, under the update seed.
//
// Parity slot: slot_ws as in eagle_sweep_kernel (candidates, mu, dist),
// plus slot_cat (2 x batch x dcat int32) for the categorical choice.
//
// Every __syncthreads must be reached by all eight waves. The sites:
//   grid_sync (two each)       top level of the iteration loop, under the
//                              grid-uniform `fold` only
//   sweep_block_reduce[2]      called from the sites below, unconditionally
//   prologue state load        under owner (blockIdx.x < batch_size)
//   phase A                    all inside the loop over b = blockIdx.x +
//                              k G, straight-line. The categorical
//                              mutation adds ONE, between the pair pass
//                              and the per-parameter scan, outside both
//                              loops (`e < n_pairs` and `j < dcat` bound
//                              arithmetic, loads and stores only)
//   vz_quadform_tile_pipelined two, outside `if (live)`
//   phase B2                   loop over q = blockIdx.x + k G
//   RC                         under owner; the categorical update adds
//                              none (it runs beside the continuous one,
//                              before the barrier that ends the reads of
//                              the old rewards)
//
// Determinism: below N = 4096 the standalone scorer takes the same tile
// quadform, so the sweep is BIT-IDENTICAL to eagle_suggest -> decode ->
// posterior_scores_chunked -> eagle_update for the same seeds
// (tests/test_sweep_mixed.py). Any grid size is correct (grid-stride
// loops); the launcher is launch_eagle_sweep's, with the grid override
// read on every call.

#include <hip/hip_runtime.h>

#include "common.h"
#include "eagle_sweep_common.h"

// Dense feature columns (xq_lds), and so categorical parameters and
// (parameter, category) pairs, a launch can have.
#define MIXED_MAX_D 512

__device__ __forceinline__ int cload_i(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cstore_i(int* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cstore_l(long long* p, long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// logit + gumbel of one (parameter, category) pair, with the roundings of
// eagle_suggest_kernel's phase 3. There the perturbation is computed
// before the loop over categories and added inside it, in another basic
// block, so the compiler cannot contract its last multiply with the add;
// here both stand in one block, so contraction is switched off.
__device__ __forceinline__ float mixed_pair_value(
    float ssum_c, bool is_cur, float scale_sum, float p_same, int size,
    float laplace, float cat_factor, float my_pert, float u) {
#pragma clang fp contract(off)
  const float logit_same = __logf(p_same);
  const float logit_diff =
      __logf((1.0f - p_same) / fmaxf((float)size - 1.0f, 1e-9f));
  const float pert_noise = laplace * cat_factor * my_pert;
  float logit = ssum_c + logit_diff;
  if (is_cur) logit += -scale_sum + logit_same - logit_diff;
  logit += pert_noise;
  const float g = -__logf(-__logf(fmaxf(u, 1e-20f)));
  return logit + g;
}

// sweep_kvec (eagle_sweep.hip) over the d dense columns, with the
// scorer's column mask: column j adds to d2 always and to the L-inf
// distance only where mask[j] == 0 (ps_kvec_kernel's `if (!onehot[j])`;
// max is exact, so skipping a column is the same in any order).
template <bool VEC4>
__device__ __forceinline__ void sweep_kvec_mixed(
    const float* __restrict__ x, const float* __restrict__ inv_ls,
    const float* __restrict__ alpha,
    const unsigned char* __restrict__ mask, const float* xq_lds,
    float* k_row, int d, int n, int wt, float amp2, float& mu_acc,
    float& min_linf) {
  for (int row0 = wt; row0 < n; row0 += KV_ROWS * BLOCK) {
    const float* xr[KV_ROWS];
    float al[KV_ROWS];
#pragma unroll
    for (int s = 0; s < KV_ROWS; ++s) {
      const int rc = min(row0 + s * BLOCK, n - 1);
      xr[s] = x + (long)rc * d;
      al[s] = alpha[rc];
    }
    float d2[KV_ROWS], linf[KV_ROWS];
#pragma unroll
    for (int s = 0; s < KV_ROWS; ++s) d2[s] = linf[s] = 0.0f;
    for (int j0 = 0; j0 < d; j0 += KV_CHUNK) {
      float cur[KV_ROWS][KV_CHUNK];
#pragma unroll
      for (int s = 0; s < KV_ROWS; ++s) {
        if (VEC4) {
          const float4 v = *reinterpret_cast<const float4*>(xr[s] + j0);
          cur[s][0] = v.x; cur[s][1] = v.y; cur[s][2] = v.z; cur[s][3] = v.w;
        } else {
#pragma unroll
          for (int c = 0; c < KV_CHUNK; ++c) {
            cur[s][c] = xr[s][min(j0 + c, d - 1)];
          }
        }
      }
      float xq[KV_CHUNK], il[KV_CHUNK];
      bool ex[KV_CHUNK];
#pragma unroll
      for (int c = 0; c < KV_CHUNK; ++c) {
        const int jc = VEC4 ? j0 + c : min(j0 + c, d - 1);
        xq[c] = xq_lds[jc];
        il[c] = inv_ls[jc];
        ex[c] = mask[jc] != 0;
      }
#pragma unroll
      for (int c = 0; c < KV_CHUNK; ++c) {
        if (VEC4 || j0 + c < d) {
#pragma unroll
          for (int s = 0; s < KV_ROWS; ++s) {
            const float diff = xq[c] - cur[s][c];
            const float z = diff * il[c];
            d2[s] = fmaf(z, z, d2[s]);
            linf[s] = ex[c] ? linf[s] : fmaxf(linf[s], fabsf(diff));
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < KV_ROWS; ++s) {
      const int row = row0 + s * BLOCK;
      const bool live = row < n;
      const float kv = amp2 * sweep_matern52(d2[s]);
      if (live) cstore(k_row + row, kv);
      mu_acc = live ? fmaf(kv, al[s], mu_acc) : mu_acc;
      min_linf = live ? fminf(min_linf, linf[s]) : min_linf;
    }
  }
}

// Whether the update improves firefly `me` (candidate i of the batch) or
// restarts it, from the old rewards and perturbations.
__device__ __forceinline__ void mixed_fate(
    const float* sc_lds, const float* st_rewards, const float* st_perts,
    int me, int i, float penalize_factor, float perturbation_lower_bound,
    float new_best, bool& improved, bool& dead) {
  const float new_r = sc_lds[i];
  const float old_r = st_rewards[me];
  improved = new_r > old_r;
  const float old_pert = st_perts[me];
  const float pert = improved ? old_pert : old_pert * penalize_factor;
  const float reward = improved ? new_r : old_r;
  dead = (pert < perturbation_lower_bound) && (reward != new_best);
}

// Compiled without packed fp32 instructions (v_pk_fma_f32 and its kin):
// every fp32 operation of this kernel is a scalar one, whatever flags the
// rest of the extension is built with.
extern "C" __global__ __launch_bounds__(SWEEP_THREADS)
__attribute__((target("no-packed-fp32-ops"))) void
eagle_sweep_mixed_kernel(
    float* __restrict__ pool_cont,         // (P, Dc)   Dc >= 0
    long long* __restrict__ pool_cat,      // (P, Dcat) Dcat >= 1
    float* __restrict__ rewards,           // (P,)
    float* __restrict__ perturbations,     // (P,)
    float* __restrict__ best_reward,       // (1,)
    unsigned long long* __restrict__ iter_ptr,  // (14,)
    unsigned int* __restrict__ barrier_buf,     // (2,) zeroed
    const float* __restrict__ x,           // (N, D)    [cached]
    const float* __restrict__ inv_ls,      // (D,)      [cached]
    const float* __restrict__ alpha,       // (N,)      [cached]
    const float* __restrict__ kinv,        // (N, N)    [cached]
    const int* __restrict__ cat_sizes,     // (Dcat,)   [cached]
    const int* __restrict__ cont_cols,     // (Dc,)     [cached]
    const int* __restrict__ cat_start,     // (Dcat,)   [cached]
    const unsigned char* __restrict__ tr_mask,  // (D,) [cached]
    float* __restrict__ out_cont,          // (B, Dc)   [wg-private]
    long long* __restrict__ out_cat,       // (B, Dcat) [wg-private]
    float* __restrict__ k_ws,              // (B, N)    [coherent]
    float* __restrict__ mu_ws,             // (B,)      [coherent]
    float* __restrict__ dist_ws,           // (B,)      [coherent]
    float* __restrict__ var_ws,            // (B, T+1)  [coherent]
    float* __restrict__ slot_ws,           // (2, B*(Dc+2)) [coherent]
    int* __restrict__ slot_cat,            // (2, B*Dcat)   [coherent]
    int n_batches, int batch_size, int pool_size, int dc, int dcat, int d,
    int max_cat, int n, long long it_start, long long iterations,
    float visibility, float gravity, float neg_gravity, float norm_scale,
    float cat_factor, float p_same, float penalize_factor,
    float perturbation_lower_bound, float base_perturbation,
    unsigned long long seed_suggest, unsigned long long seed_update,
    float amp2, float mean_c, int acq, float coef, float best_value,
    float tr_radius) {
  __shared__ float scale[MAX_POOL];
  __shared__ float red[8];
  __shared__ float red2[4];  // second value of sweep_block_reduce2
  __shared__ float s_scalar;
  __shared__ __attribute__((aligned(16))) float xq_lds[MIXED_MAX_D];
  // Lower half: phase B's staging of half 0, RC's scratch, and phase A's
  // pair values and categorical choice. Upper half: the continuous pool.
  __shared__ float pool_lds[POOL_LDS_CAP];
  __shared__ float stage1_lds[2 * VZ_QF_QMAX * VZ_QF_TILE];
  __shared__ float st_rewards[MAX_POOL];
  __shared__ float st_perts[MAX_POOL];
  __shared__ float st_best;
  // The categorical half of the state and the parameter tables.
  __shared__ unsigned short st_cat[RESIDENT_CAT_CAP];
  __shared__ unsigned short tab_size[MIXED_MAX_D];    // per parameter
  __shared__ unsigned short tab_base[MIXED_MAX_D];    // its first pair
  __shared__ unsigned short tab_start[MIXED_MAX_D];   // its first column
  __shared__ unsigned short pair_param[MIXED_MAX_D];  // per pair

  const int tid = threadIdx.x;
  const int half = tid / BLOCK;
  const int htid = tid % BLOCK;
  const int wt = half == 0 ? tid : SWEEP_IDLE;
  const int G = gridDim.x;
  const int pool_elems = pool_size * dc;
  const int cat_elems = pool_size * dcat;
  const int n_pairs = d - dc;  // the binding checks sum(cat_sizes) == d - dc
  const int n_features = dc + dcat;
  const bool owner = blockIdx.x < batch_size;
  const bool x_vec4 = d % KV_CHUNK == 0 &&
                      (reinterpret_cast<unsigned long long>(x) & 15) == 0;
  float* st_pool = pool_lds + RESIDENT_CAP;
  // Phase A scratch in the lower half of pool_lds (free until phase B).
  float* pair_val = pool_lds;
  auto fsum = [](float a, float c) { return a + c; };
  auto fmin_ = [](float a, float c) { return fminf(a, c); };

  // Per-phase ticks as in eagle_sweep_kernel: iter_ptr[2..9] are A, barA,
  // B, barB, B2, barB2, RC, (unused); [10..11] phase B's stage / main;
  // [12] the categorical mutation inside A (pair pass, its barrier and
  // the per-parameter scan, as thread 0 of workgroup 0 sees them).
  const bool profwg = (blockIdx.x == 0 && threadIdx.x == 0);
  unsigned long long tmark = profwg ? wall_clock64() : 0;
  unsigned int bar_target = 0;
#define VZ_SWEEP_PROF(slot)                                        \
  if (profwg) {                                                    \
    const unsigned long long tnow = wall_clock64();                \
    iter_ptr[2 + (slot)] += tnow - tmark;                          \
    tmark = tnow;                                                  \
  }

  // The state was written by earlier launches, so plain loads see it;
  // from here on only this workgroup touches its copy.
  if (owner) {
    for (int e = wt; e < pool_elems; e += BLOCK) st_pool[e] = pool_cont[e];
    for (int e = wt; e < cat_elems; e += BLOCK) {
      st_cat[e] = (unsigned short)pool_cat[e];
    }
    for (int p = wt; p < pool_size; p += BLOCK) {
      st_rewards[p] = rewards[p];
      st_perts[p] = perturbations[p];
    }
    for (int j = wt; j < dcat; j += BLOCK) {
      int base = 0;
      for (int i = 0; i < j; ++i) base += cat_sizes[i];
      const int size = cat_sizes[j];
      tab_size[j] = (unsigned short)size;
      tab_base[j] = (unsigned short)base;
      tab_start[j] = (unsigned short)cat_start[j];
      for (int c = 0; c < size; ++c) pair_param[base + c] = (unsigned short)j;
    }
    if (tid == 0) st_best = best_reward[0];
    __syncthreads();
  }

  for (long long it = it_start; it < it_start + iterations; ++it) {
    const unsigned long long offset = (unsigned long long)it;
    // Parity slot of this iteration: candidates, then mu, then dist; and
    // the categorical choice.
    float* slot_c = slot_ws + (long)(it & 1) * batch_size * (dc + 2);
    float* slot_mu = slot_c + batch_size * dc;
    float* slot_dist = slot_mu + batch_size;
    int* slot_k = slot_cat + (long)(it & 1) * batch_size * dcat;
    const int batch_start =
        (int)(offset % (unsigned long long)n_batches) * batch_size;
    if (profwg) tmark = wall_clock64();

    // ---- Phase A: suggest + k-vec (workgroup owns candidate b) ----
    for (int b = blockIdx.x; b < batch_size; b += G) {
      const int me = batch_start + b;
      const float my_reward = st_rewards[me];
      const float my_pert = st_perts[me];
      for (int p = wt; p < pool_size; p += BLOCK) {
        // The continuous chain j = 0 .. dc - 1, SG_DCHUNK loads at a time.
        float d2 = 0.0f;
        for (int j0 = 0; j0 < dc; j0 += SG_DCHUNK) {
          float mv[SG_DCHUNK], pv[SG_DCHUNK];
#pragma unroll
          for (int u = 0; u < SG_DCHUNK; ++u) {
            const int jc = min(j0 + u, dc - 1);
            mv[u] = st_pool[me * dc + jc];
            pv[u] = st_pool[p * dc + jc];
          }
#pragma unroll
          for (int u = 0; u < SG_DCHUNK; ++u) {
            const float diff = mv[u] - pv[u];
            d2 = (j0 + u < dc) ? fmaf(diff, diff, d2) : d2;
          }
        }
        // Then the Hamming count, one rounded + 1 per differing column
        // in the order j = 0 .. dcat - 1 (d2 + 0 is d2).
        for (int j0 = 0; j0 < dcat; j0 += SG_DCHUNK) {
          unsigned short mc[SG_DCHUNK], pc[SG_DCHUNK];
#pragma unroll
          for (int u = 0; u < SG_DCHUNK; ++u) {
            const int jc = min(j0 + u, dcat - 1);
            mc[u] = st_cat[me * dcat + jc];
            pc[u] = st_cat[p * dcat + jc];
          }
#pragma unroll
          for (int u = 0; u < SG_DCHUNK; ++u) {
            d2 = (j0 + u < dcat && mc[u] != pc[u]) ? d2 + 1.0f : d2;
          }
        }
        const float reward_p = st_rewards[p];
        const float dir = (reward_p - my_reward >= 0.0f) ? gravity
                                                         : -neg_gravity;
        const float force = __expf(-visibility * d2 / n_features * 10.0f);
        float s = dir * force;
        if (!isfinite(reward_p)) s = 0.0f;
        scale[p] = s;
      }
      __syncthreads();
      float pulls = 0.0f, pushes = 0.0f;
      for (int p = wt; p < pool_size; p += BLOCK) {
        pulls += (scale[p] > 0.0f) ? 1.0f : 0.0f;
        pushes += (scale[p] < 0.0f) ? 1.0f : 0.0f;
      }
      sweep_block_reduce2(pulls, pushes, red, red2, fsum, fsum, 0.0f, 0.0f);
      if (tid == 0) {
        red[4] = fmaxf(pulls, 1.0f);
        red[5] = fmaxf(pushes, 1.0f);
      }
      __syncthreads();
      const float inv_pull = 1.0f / red[4];
      const float inv_push = 1.0f / red[5];
      float ssum = 0.0f;
      for (int p = wt; p < pool_size; p += BLOCK) {
        const float s = scale[p];
        const float ns = norm_scale * (s > 0.0f ? s * inv_pull
                                                : s * inv_push);
        scale[p] = ns;
        ssum += ns;
      }
      __syncthreads();
      float scale_sum = sweep_block_reduce(ssum, red, fsum, 0.0f);
      if (tid == 0) s_scalar = scale_sum;
      __syncthreads();
      scale_sum = s_scalar;

      // Continuous move, into the dense column of the parameter.
      for (int j = wt; j < dc; j += BLOCK) {
        const int col = cont_cols[j];
        float moved = 0.0f;
        for (int p0 = 0; p0 < pool_size; p0 += SG_PCHUNK) {
          float sv[SG_PCHUNK], pv[SG_PCHUNK];
#pragma unroll
          for (int u = 0; u < SG_PCHUNK; ++u) {
            const int pc = min(p0 + u, pool_size - 1);
            sv[u] = scale[pc];
            pv[u] = st_pool[pc * dc + j];
          }
#pragma unroll
          for (int u = 0; u < SG_PCHUNK; ++u) {
            moved = (p0 + u < pool_size) ? fmaf(sv[u], pv[u], moved)
                                         : moved;
          }
        }
        const float mine = st_pool[me * dc + j];
        moved = mine + (moved - mine * scale_sum);
        float noise = vz_rng_laplace<float>(seed_suggest, offset,
                                            (unsigned)(b * dc + j));
        noise = (noise >= 0.0f) ? 1.0f : -1.0f;  // q == 1
        const float cand = moved + noise * my_pert;
        out_cont[b * dc + j] = cand;
        cstore(slot_c + b * dc + j, cand);
        xq_lds[col] = cand;
      }

      // Categorical mutation, pair pass: thread e owns (parameter j,
      // category c).
      const unsigned long long tcat = profwg ? wall_clock64() : 0;
      for (int e = wt; e < n_pairs; e += BLOCK) {
        const int j = pair_param[e];
        const int c = e - tab_base[j];
        float ssum_c = 0.0f;
        for (int p0 = 0; p0 < pool_size; p0 += SG_PCHUNK) {
          float sv[SG_PCHUNK];
          unsigned short cv[SG_PCHUNK];
#pragma unroll
          for (int u = 0; u < SG_PCHUNK; ++u) {
            const int pc = min(p0 + u, pool_size - 1);
            sv[u] = scale[pc];
            cv[u] = st_cat[pc * dcat + j];
          }
#pragma unroll
          for (int u = 0; u < SG_PCHUNK; ++u) {
            ssum_c = (p0 + u < pool_size && cv[u] == c) ? ssum_c + sv[u]
                                                        : ssum_c;
          }
        }
        const unsigned idx = (unsigned)(b * dcat + j);
        const float laplace = vz_rng_laplace<float>(
            seed_suggest, offset ^ 0x9e01ull, idx);
        const float u01 = vz_rng_uniform<float>(
            seed_suggest, offset ^ 0x77aaull,
            (unsigned)((b * dcat + j) * max_cat + c));
        pair_val[e] = mixed_pair_value(
            ssum_c, c == (int)st_cat[me * dcat + j], scale_sum, p_same,
            tab_size[j], laplace, cat_factor, my_pert, u01);
      }
      __syncthreads();  // the one barrier the mutation adds
      // Per-parameter argmax: strict > from c = 0, the step kernel's scan.
      for (int j = wt; j < dcat; j += BLOCK) {
        const int size = tab_size[j];
        const float* vals = pair_val + tab_base[j];
        float best_val = -INFINITY;
        int best_cat = st_cat[me * dcat + j];
        for (int c = 0; c < size; ++c) {
          const float v = vals[c];
          if (v > best_val) {
            best_val = v;
            best_cat = c;
          }
        }
        out_cat[b * dcat + j] = best_cat;
        cstore_i(slot_k + b * dcat + j, best_cat);
        float* block = xq_lds + tab_start[j];
        for (int c = 0; c < size; ++c) block[c] = (c == best_cat) ? 1.0f : 0.0f;
      }
      if (profwg) iter_ptr[12] += wall_clock64() - tcat;
      __syncthreads();

      // k-vector + mu + trust-region distance over the dense columns.
      float mu_acc = 0.0f;
      float min_linf = INFINITY;
      if (x_vec4) {
        sweep_kvec_mixed<true>(x, inv_ls, alpha, tr_mask, xq_lds,
                               k_ws + (long)b * n, d, n, wt, amp2, mu_acc,
                               min_linf);
      } else {
        sweep_kvec_mixed<false>(x, inv_ls, alpha, tr_mask, xq_lds,
                                k_ws + (long)b * n, d, n, wt, amp2, mu_acc,
                                min_linf);
      }
      sweep_block_reduce2(mu_acc, min_linf, red, red2, fsum, fmin_, 0.0f,
                          INFINITY);
      if (tid == 0) {
        cstore(mu_ws + b, mu_acc);
        cstore(dist_ws + b, min_linf);
        cstore(slot_mu + b, mu_acc);
        cstore(slot_dist + b, min_linf);
      }
      __syncthreads();
    }
    VZ_SWEEP_PROF(0)
    grid_sync(barrier_buf, bar_target);
    VZ_SWEEP_PROF(1)

    // ---- Phase B: K^-1 quadform, as eagle_sweep_kernel ----
    const int tiles_n = (n + VZ_QF_TILE - 1) / VZ_QF_TILE;
    const int total_tiles = tiles_n * tiles_n;
    {
      float* k_i_lds = half == 0 ? pool_lds : stage1_lds;
      float* k_j_lds = k_i_lds + VZ_QF_QMAX * VZ_QF_TILE;
      for (int tile0 = blockIdx.x; tile0 < total_tiles; tile0 += 2 * G) {
        const int t = tile0 + half * G;
        vz_quadform_tile_pipelined(
            kinv, batch_size, n, t, tiles_n, htid, t < total_tiles,
            k_i_lds, k_j_lds,
            [&](long idx) { return cload(k_ws + idx); },
            [&](int q, float v) {
              cstore(var_ws + (long)q * (total_tiles + 1) + t, v);
            },
            blockIdx.x == 0 ? iter_ptr + 10 : nullptr);
      }
    }
    VZ_SWEEP_PROF(2)
    grid_sync(barrier_buf, bar_target);
    VZ_SWEEP_PROF(3)

    // ---- Phase B2: only above FOLD_MAX_TILES, as eagle_sweep_kernel ----
    const bool fold = total_tiles <= FOLD_MAX_TILES;  // grid-uniform
    if (!fold) {
      for (int q = blockIdx.x; q < batch_size; q += G) {
        float sacc = 0.0f;
        for (int w = wt; w < total_tiles; w += BLOCK) {
          sacc += cload(var_ws + (long)q * (total_tiles + 1) + w);
        }
        float total = sweep_block_reduce(sacc, red, fsum, 0.0f);
        if (tid == 0) {
          cstore(var_ws + (long)q * (total_tiles + 1) + total_tiles, total);
        }
        __syncthreads();
      }
      VZ_SWEEP_PROF(4)
      grid_sync(barrier_buf, bar_target);
      VZ_SWEEP_PROF(5)
    }

    // ---- RC: reduce (when folded) + scores + update of both halves ----
    if (owner) {
      float* wp = pool_lds;
      float* sc_lds = pool_lds + 4 * VZ_QF_QMAX;
      float mu_t = 0.0f, dist_t = 0.0f;
      if (tid < batch_size) {
        mu_t = cload(slot_mu + tid);
        dist_t = cload(slot_dist + tid);
      }
      if (fold && half == 0) {
        reduce_all_partials(var_ws, batch_size, total_tiles, wp);
      }
      __syncthreads();
      if (tid < WAVE_SIZE) {  // batch <= VZ_QF_QMAX < WAVE_SIZE
        float score = -INFINITY;
        if (tid < batch_size) {
          float* reduced =
              var_ws + (long)tid * (total_tiles + 1) + total_tiles;
          float quad;
          if (fold) {
            quad = fold_quad(wp, tid);
            if (tid % G == (int)blockIdx.x) cstore(reduced, quad);
          } else {
            quad = cload(reduced);
          }
          float var = fmaxf(amp2 - quad, 1e-12f);
          const float sd = sqrtf(var);
          const float mu = mu_t + mean_c;
          score = vz_trust_region(
              vz_acq_score(acq, mu, sd, coef, best_value), dist_t,
              tr_radius);
          sc_lds[tid] = score;
        }
        const float batch_max = wave_reduce_max(score);
        if (tid == 0) s_scalar = fmaxf(st_best, batch_max);
      }
      __syncthreads();
      const float new_best = s_scalar;
      for (int e = wt; e < batch_size * dc; e += BLOCK) {
        const int i = e / dc;
        const int me = batch_start + i;
        const int ej = me * dc + (e - i * dc);
        bool improved, dead;
        mixed_fate(sc_lds, st_rewards, st_perts, me, i, penalize_factor,
                   perturbation_lower_bound, new_best, improved, dead);
        if (dead) {
          st_pool[ej] = vz_rng_uniform<float>(
              seed_update, offset ^ 0x5151ull, (unsigned)ej);
        } else if (improved) {
          st_pool[ej] = cload(slot_c + e);
        }
      }
      for (int e = wt; e < batch_size * dcat; e += BLOCK) {
        const int i = e / dcat;
        const int j = e - i * dcat;
        const int me = batch_start + i;
        const int ej = me * dcat + j;
        bool improved, dead;
        mixed_fate(sc_lds, st_rewards, st_perts, me, i, penalize_factor,
                   perturbation_lower_bound, new_best, improved, dead);
        if (dead) {
          const long size = tab_size[j];
          const float u = vz_rng_uniform<float>(
              seed_update, offset ^ 0x1234ull, (unsigned)ej);
          const long c = (long)(u * (float)size);
          st_cat[ej] = (unsigned short)min(c, size - 1);
        } else if (improved) {
          st_cat[ej] = (unsigned short)cload_i(slot_k + e);
        }
      }
      __syncthreads();  // every read of the old rewards / perts is done
      if (tid < batch_size) {
        const int me = batch_start + tid;
        const float new_r = sc_lds[tid];
        const float old_r = st_rewards[me];
        const bool improved = new_r > old_r;
        const float old_pert = st_perts[me];
        float pert = improved ? old_pert : old_pert * penalize_factor;
        float reward = improved ? new_r : old_r;
        const bool dead = (pert < perturbation_lower_bound) &&
                          (reward != new_best);
        if (dead) {
          reward = -INFINITY;
          pert = base_perturbation;
        }
        st_rewards[me] = reward;
        st_perts[me] = pert;
      }
      if (tid == 0) st_best = new_best;
      __syncthreads();
    }
    VZ_SWEEP_PROF(6)
  }

  // Every owner holds the same final state; workgroup 0 hands both halves
  // back. With iterations == 0 nothing changed.
  if (blockIdx.x == 0 && iterations > 0) {
    for (int e = wt; e < pool_elems; e += BLOCK) {
      cstore(pool_cont + e, st_pool[e]);
    }
    for (int e = wt; e < cat_elems; e += BLOCK) {
      cstore_l(pool_cat + e, (long long)st_cat[e]);
    }
    for (int p = wt; p < pool_size; p += BLOCK) {
      cstore(rewards + p, st_rewards[p]);
      cstore(perturbations + p, st_perts[p]);
    }
    if (tid == 0) cstore(best_reward, st_best);
  }

  if (blockIdx.x == 0 && tid == 0) {
    iter_ptr[0] = (unsigned long long)(it_start + iterations);
    iter_ptr[1] = (unsigned long long)(it_start + iterations - 1);
  }
}

// Host launcher: launch_eagle_sweep's grid rule and its fall-back to an
// ordinary launch where the device's one cooperative queue belongs to
// another process (see eagle_sweep.hip). VIZIER_AMD_SWEEP_GRID is read on
// every call here. Returns the grid size used, 0 if cooperative launch is
// unavailable, or a negative hipError_t on failure.
extern "C" int launch_eagle_sweep_mixed(
    float* pool_cont, long long* pool_cat, float* rewards,
    float* perturbations, float* best_reward, unsigned long long* iter_ptr,
    unsigned int* barrier_buf, const float* x, const float* inv_ls,
    const float* alpha, const float* kinv, const int* cat_sizes,
    const int* cont_cols, const int* cat_start,
    const unsigned char* tr_mask, float* out_cont, long long* out_cat,
    float* k_ws, float* mu_ws, float* dist_ws, float* var_ws,
    float* slot_ws, int* slot_cat, int n_batches, int batch_size,
    int pool_size, int dc, int dcat, int d, int max_cat, int n,
    long long it_start, long long iterations, float visibility,
    float gravity, float neg_gravity, float norm_scale, float cat_factor,
    float p_same, float penalize_factor, float perturbation_lower_bound,
    float base_perturbation, unsigned long long seed_suggest,
    unsigned long long seed_update, float amp2, float mean_c, int acq,
    float coef, float best_value, float tr_radius, hipStream_t stream) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  int coop = 0;
  (void)hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch,
                              dev);
  if (!coop) return 0;
  int num_cu = 0;
  (void)hipDeviceGetAttribute(&num_cu,
                              hipDeviceAttributeMultiprocessorCount, dev);
  int blocks_per_cu = 0;
  hipError_t err = hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &blocks_per_cu, (const void*)eagle_sweep_mixed_kernel, SWEEP_THREADS,
      0);
  if (err != hipSuccess || blocks_per_cu < 1) return 0;
  const int tiles_n = (n + VZ_QF_TILE - 1) / VZ_QF_TILE;
  int grid = tiles_n * tiles_n;  // fills phase B
  if (grid > 128) grid = 128;
  if (grid < 64) grid = 64;
  const char* env = getenv("VIZIER_AMD_SWEEP_GRID");
  const int grid_env = (env != nullptr) ? atoi(env) : 0;
  if (grid_env > 0) grid = grid_env;
  const int max_grid = blocks_per_cu * num_cu;
  if (grid > max_grid) grid = max_grid;
  if (grid < 1) grid = 1;

  void* args[] = {
      &pool_cont, &pool_cat, &rewards, &perturbations, &best_reward,
      &iter_ptr, &barrier_buf, &x, &inv_ls, &alpha, &kinv, &cat_sizes,
      &cont_cols, &cat_start, &tr_mask, &out_cont, &out_cat, &k_ws, &mu_ws,
      &dist_ws, &var_ws, &slot_ws, &slot_cat, &n_batches, &batch_size,
      &pool_size, &dc, &dcat, &d, &max_cat, &n, &it_start, &iterations,
      &visibility, &gravity, &neg_gravity, &norm_scale, &cat_factor,
      &p_same, &penalize_factor, &perturbation_lower_bound,
      &base_perturbation, &seed_suggest, &seed_update, &amp2, &mean_c, &acq,
      &coef, &best_value, &tr_radius};
  err = hipLaunchCooperativeKernel((const void*)eagle_sweep_mixed_kernel,
                                   dim3(grid), dim3(SWEEP_THREADS), args, 0,
                                   stream);
  if (err == hipErrorIllegalState) {
    // No cooperative queue for this process and nothing was enqueued: the
    // same grid, already clamped to what the device holds at once, as an
    // ordinary launch. launch_eagle_sweep says why that is enough.
    (void)hipGetLastError();
    err = hipLaunchKernel((const void*)eagle_sweep_mixed_kernel, dim3(grid),
                          dim3(SWEEP_THREADS), args, 0, stream);
  }
  if (err != hipSuccess) return -(int)err;
  return grid;
}
