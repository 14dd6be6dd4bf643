// Persistent cooperative Eagle-sweep megakernel for multi-objective
// studies on gfx950: M independent Matern-5/2 GPs on ONE training set x,
// scored by hypervolume scalarisation. Continuous spaces, q == 1, fp32.
//
// The hipGraph path replays, per iteration, eagle_suggest, then per metric
// the three kernels of posterior_mean_std, two stack copies,
// hv_scalarize_tr and eagle_update: about 5 + 3 M dependent launches. This
// kernel runs the whole steady-state sweep in one launch, in the resident
// form of eagle_sweep.hip (read its header first: the coherence design,
// grid_sync on one growing counter, cload / cstore for the small
// inter-phase buffers, the state private to every owning workgroup in
// LDS, the parity slots). There is no legacy form: the binding rejects
// pool_size * dc > RESIDENT_CAP.
//
// How M metrics share one iteration (two grid barriers: A | B | RC):
//
//   A   The owner of candidate b runs the suggest step of eagle_sweep.hip,
//       then ONE pass over the rows of x (sweep_kvec_mo). A row is loaded
//       once and its differences xq - x are formed once; metric m scales
//       them by its own inv_ls[m] into its own squared-distance chain, so
//       the loads, the subtractions and the masked L-inf distance (which
//       does not depend on the metric) are paid once where the step path
//       pays them M times. Per metric the chain is sweep_kvec's, hence
//       ps_kvec_kernel's: k_ws (M, b, n) holds the bits posterior_mean_std
//       produces for posterior m. The M mean sums and the distance go
//       through one barrier pass (mo_block_reduce: M + 1 shuffle trees,
//       each block_reduce's, on LDS slots of their own).
//
//   B   One list of M * T * T items (T = ceil(n / 64)): item m * T * T + t
//       is tile t of K_inv[m] against the k slabs of metric m. Item
//       blockIdx.x + G * (2 * trip + half) goes to half `half` of the
//       workgroup, as the T * T tiles of eagle_sweep.hip do, so a trip may
//       hold tiles of two metrics, and the halves of one workgroup may
//       work on different metrics. Partials go to var_ws (M, b, T*T + 1).
//
//   RC  reduce + scalarise + update, on every owning workgroup, with NO
//       third barrier: every owner recomputes all b scores. Decision and
//       cost: an owner needs all b scores for the update anyway; giving
//       each owner only its own candidate's scalarisation would need the
//       scores handed over through one more grid barrier. Recomputed, the
//       scalarisation costs ceil(b / 2) * ceil(S / 256) * M divisions per
//       thread (104 at b = 25, S = 1000, M = 2) and ONE __syncthreads,
//       because the two halves of the workgroup take alternate candidates
//       (and alternate metrics in the reduce), each half doing the
//       256-thread arithmetic of the step kernels:
//         1. metric m's tile partials are reduced by half m & 1, for all
//            candidates at once (reduce_all_partials_at: B2's order);
//         2. thread q < b folds them, forms mean_m, sd_m and
//            y_m = mean_m + coef * sd_m - ref[m] for every metric m;
//         3. candidate c is scalarised by half c & 1: 256 threads stride
//            over the S weight vectors, v = min_m y_m / w[s, m], in
//            hv_scalarize_tr_kernel's order; the four wave partials of a
//            candidate are left in LDS;
//         4. thread q < b folds its candidate's four wave partials in
//            block_reduce's order, divides by S and applies the
//            trust-region cut-off;
//         5. the update of all b fireflies of eagle_sweep.hip's RC.
//       profiles/bench_sweep_mo.md has the measured cost of RC against
//       that of a grid barrier.
//
// weights (S, M) and ref are read-only. An owner stages the weights in LDS
// once per launch when S * M <= MO_W_LDS; otherwise they are read on the
// cached path in every iteration.
//
// Parity slots: slot it & 1 of slot_ws holds the candidates (b, dc), the
// M mean sums (M, b) and the distance (b) of iteration it, for the reason
// given in eagle_sweep.hip. out_cont, mu_ws, dist_ws, ms_ws and score_ws
// are written for the caller only (the tests); the kernel does not read
// them.
//
// Every __syncthreads is reached by all eight waves. The sites:
//   grid_sync (two)            top level of the iteration loop
//   prologue state load        under owner (blockIdx.x < batch_size)
//   phase A                    inside the loop over b = blockIdx.x + k G,
//                              straight-line; mo_block_reduce has one
//   vz_quadform_tile_pipelined two, outside `if (live)`; the trip loop runs
//                              on item0 = blockIdx.x + 2 G trip, the same
//                              for both halves
//   RC                         five, under owner only; the conditions on
//                              `half`, `live`, `tid` and `lane` enclose
//                              loads, stores, shuffles and arithmetic only
// Any grid size is correct: every phase is a grid-stride loop, a workgroup
// past the batch owns nothing and only takes part in B and the barriers,
// and with a grid below the batch A loops over its candidates and RC runs
// once per workgroup.
//
// Determinism: every value comes from the operations of the step kernels
// on the same operands in the same order, so the sweep is BIT-IDENTICAL
// to eagle_suggest -> posterior_mean_std per metric -> hv_scalarize_tr ->
// eagle_update for n < 4096 (from 4096 the standalone scorer takes its
// SGEMM route; the binding rejects that range). tests/test_sweep_mo.py.

#include <hip/hip_runtime.h>

#include "common.h"
#include "eagle_sweep_common.h"

#define MO_MAX_M 4
// Floats of the weights an owner keeps in LDS (8 KiB): S = 1000 at M = 2.
#define MO_W_LDS 2048

// The per-metric operands that are not shared: passed by value, indexed by
// unrolled loops only (a dynamic index would put the struct in scratch).
struct MoMetrics {
  const float* kinv[MO_MAX_M];  // (N, N) each  [cached]
  float amp2[MO_MAX_M];
  float mean_c[MO_MAX_M];
};

// sweep_kvec (eagle_sweep.hip) for M metrics in one pass over x: the rows,
// the candidate and the mask are loaded once and diff = xq - x is formed
// once; metric m then runs sweep_kvec's chain on it (z = diff * inv_ls[m],
// d2 = fma(z, z, d2), row by row, j = 0 .. dc - 1). The L-inf distance
// skips the columns with mask[j] != 0 (ps_kvec_kernel's `if (!onehot[j])`).
template <int M, bool VEC4>
__device__ __forceinline__ void sweep_kvec_mo(
    const float* __restrict__ x, const float* __restrict__ inv_ls,
    const float* __restrict__ alpha, const unsigned char* __restrict__ mask,
    const float* xq_lds, float* k_ws, long k_stride, int dc, int n, int wt,
    const MoMetrics& P, float (&mu_acc)[M], float& min_linf) {
  for (int row0 = wt; row0 < n; row0 += KV_ROWS * BLOCK) {
    const float* xr[KV_ROWS];
    float al[M][KV_ROWS];
#pragma unroll
    for (int s = 0; s < KV_ROWS; ++s) {
      const int rc = min(row0 + s * BLOCK, n - 1);
      xr[s] = x + (long)rc * dc;
#pragma unroll
      for (int m = 0; m < M; ++m) al[m][s] = alpha[(long)m * n + rc];
    }
    float d2[M][KV_ROWS], linf[KV_ROWS];
#pragma unroll
    for (int s = 0; s < KV_ROWS; ++s) {
      linf[s] = 0.0f;
#pragma unroll
      for (int m = 0; m < M; ++m) d2[m][s] = 0.0f;
    }
    for (int j0 = 0; j0 < dc; j0 += KV_CHUNK) {
      float cur[KV_ROWS][KV_CHUNK];
#pragma unroll
      for (int s = 0; s < KV_ROWS; ++s) {
        if (VEC4) {
          const float4 v = *reinterpret_cast<const float4*>(xr[s] + j0);
          cur[s][0] = v.x; cur[s][1] = v.y; cur[s][2] = v.z; cur[s][3] = v.w;
        } else {
#pragma unroll
          for (int c = 0; c < KV_CHUNK; ++c) {
            cur[s][c] = xr[s][min(j0 + c, dc - 1)];
          }
        }
      }
      float xq[KV_CHUNK], il[M][KV_CHUNK];
      bool ex[KV_CHUNK];
#pragma unroll
      for (int c = 0; c < KV_CHUNK; ++c) {
        const int jc = VEC4 ? j0 + c : min(j0 + c, dc - 1);
        xq[c] = xq_lds[jc];
        ex[c] = mask[jc] != 0;
#pragma unroll
        for (int m = 0; m < M; ++m) il[m][c] = inv_ls[m * dc + jc];
      }
#pragma unroll
      for (int c = 0; c < KV_CHUNK; ++c) {
        if (VEC4 || j0 + c < dc) {
#pragma unroll
          for (int s = 0; s < KV_ROWS; ++s) {
            const float diff = xq[c] - cur[s][c];
#pragma unroll
            for (int m = 0; m < M; ++m) {
              const float z = diff * il[m][c];
              d2[m][s] = fmaf(z, z, d2[m][s]);
            }
            linf[s] = ex[c] ? linf[s] : fmaxf(linf[s], fabsf(diff));
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < KV_ROWS; ++s) {
      const int row = row0 + s * BLOCK;
      const bool live = row < n;
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const float kv = P.amp2[m] * sweep_matern52(d2[m][s]);
        if (live) cstore(k_ws + m * k_stride + row, kv);
        mu_acc[m] = live ? fmaf(kv, al[m][s], mu_acc[m]) : mu_acc[m];
      }
      min_linf = live ? fminf(min_linf, linf[s]) : min_linf;
    }
  }
}

// M sums and one min on one barrier pass: each value goes through
// sweep_block_reduce's shuffle tree and second stage on LDS slots of its
// own (lds: (M + 1) x 4 floats), so each has the bits of a block_reduce
// of its own. Results in place, valid in thread 0.
template <int M>
__device__ __forceinline__ void mo_block_reduce(float (&sums)[M], float& mn,
                                                float* lds) {
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
#pragma unroll
  for (int offset = WAVE_SIZE / 2; offset > 0; offset >>= 1) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      sums[m] = sums[m] + __shfl_down(sums[m], offset, WAVE_SIZE);
    }
    mn = fminf(mn, __shfl_down(mn, offset, WAVE_SIZE));
  }
  if (lane == 0 && wave < BLOCK / WAVE_SIZE) {
#pragma unroll
    for (int m = 0; m < M; ++m) lds[4 * m + wave] = sums[m];
    lds[4 * M + wave] = mn;
  }
  __syncthreads();
  if (wave == 0) {
    const bool in = lane < BLOCK / WAVE_SIZE;
#pragma unroll
    for (int m = 0; m < M; ++m) sums[m] = in ? lds[4 * m + lane] : 0.0f;
    mn = in ? lds[4 * M + lane] : INFINITY;
#pragma unroll
    for (int offset = 2; offset > 0; offset >>= 1) {
#pragma unroll
      for (int m = 0; m < M; ++m) {
        sums[m] = sums[m] + __shfl_down(sums[m], offset, WAVE_SIZE);
      }
      mn = fminf(mn, __shfl_down(mn, offset, WAVE_SIZE));
    }
  }
}

// Compiled without packed fp32 instructions, as eagle_sweep_mixed_kernel.
template <int M>
__global__ __launch_bounds__(SWEEP_THREADS)
__attribute__((target("no-packed-fp32-ops"))) void
eagle_sweep_mo_kernel(
    float* __restrict__ pool_cont,         // (P, Dc)
    float* __restrict__ rewards,           // (P,)
    float* __restrict__ perturbations,     // (P,)
    float* __restrict__ best_reward,       // (1,)
    unsigned long long* __restrict__ iter_ptr,  // (12,)
    unsigned int* __restrict__ barrier_buf,     // (2,) zeroed
    const float* __restrict__ x,           // (N, Dc)    [cached]
    const float* __restrict__ inv_ls,      // (M, Dc)    [cached]
    const float* __restrict__ alpha,       // (M, N)     [cached]
    const MoMetrics P,                     // K_inv, amp2, mean_c per metric
    const float* __restrict__ weights,     // (S, M)     [cached]
    const float* __restrict__ ref,         // (M,) or null [cached]
    const unsigned char* __restrict__ tr_mask,  // (Dc,) [cached]
    float* __restrict__ out_cont,          // (B, Dc)    [wg-private]
    float* __restrict__ k_ws,              // (M, B, N)  [coherent]
    float* __restrict__ mu_ws,             // (M, B)     [caller]
    float* __restrict__ dist_ws,           // (B,)       [caller]
    float* __restrict__ var_ws,            // (M, B, T*T+1) [coherent]
    float* __restrict__ ms_ws,             // (2, M, B) mean, sd [caller]
    float* __restrict__ score_ws,          // (B,)       [caller]
    float* __restrict__ slot_ws,           // (2, B*(Dc+M+1)) [coherent]
    int n_batches, int batch_size, int pool_size, int dc, int n, int n_scal,
    long long it_start, long long iterations,
    float visibility, float gravity, float neg_gravity, float norm_scale,
    float penalize_factor, float perturbation_lower_bound,
    float base_perturbation,
    unsigned long long seed_suggest, unsigned long long seed_update,
    float coef, float tr_radius) {
  __shared__ float scale[MAX_POOL];
  __shared__ float red[8];
  __shared__ float red2[4];
  __shared__ float red_mo[4 * (MO_MAX_M + 1)];
  __shared__ float s_scalar;
  __shared__ __attribute__((aligned(16))) float xq_lds[512];
  // Lower half: phase B's staging of half 0 and RC's scratch. Upper half:
  // this workgroup's copy of the pool.
  __shared__ float pool_lds[POOL_LDS_CAP];
  __shared__ float stage1_lds[2 * VZ_QF_QMAX * VZ_QF_TILE];
  __shared__ float st_rewards[MAX_POOL];
  __shared__ float st_perts[MAX_POOL];
  __shared__ float st_best;
  __shared__ float w_lds[MO_W_LDS];

  const int tid = threadIdx.x;
  const int half = tid / BLOCK;
  const int htid = tid % BLOCK;
  const int wt = half == 0 ? tid : SWEEP_IDLE;
  const int G = gridDim.x;
  const int pool_elems = pool_size * dc;
  const bool owner = blockIdx.x < batch_size;
  const bool x_vec4 = dc % KV_CHUNK == 0 &&
                      (reinterpret_cast<unsigned long long>(x) & 15) == 0;
  const bool w_staged = n_scal * M <= MO_W_LDS;  // grid-uniform
  // The weights RC reads: the LDS copy or the cached path.
  const float* wsrc = w_staged ? w_lds : weights;
  float* st_pool = pool_lds + RESIDENT_CAP;
  const int tiles_n = (n + VZ_QF_TILE - 1) / VZ_QF_TILE;
  const int total_tiles = tiles_n * tiles_n;
  const int total_items = M * total_tiles;
  const long k_stride = (long)batch_size * n;                 // per metric
  const long var_stride = (long)batch_size * (total_tiles + 1);
  auto fsum = [](float a, float c) { return a + c; };

  // Per-phase cycle profiling, as eagle_sweep.hip: iter_ptr[2..9] are
  // A, barA, B, barB, -, -, RC, -; [10..11] phase B's staging / compute.
  const bool profwg = (blockIdx.x == 0 && threadIdx.x == 0);
  unsigned long long tmark = profwg ? wall_clock64() : 0;
  unsigned int bar_target = 0;
#define VZ_SWEEP_PROF(slot)                                        \
  if (profwg) {                                                    \
    const unsigned long long tnow = wall_clock64();                \
    iter_ptr[2 + (slot)] += tnow - tmark;                          \
    tmark = tnow;                                                  \
  }

  if (owner) {
    for (int e = wt; e < pool_elems; e += BLOCK) st_pool[e] = pool_cont[e];
    for (int p = wt; p < pool_size; p += BLOCK) {
      st_rewards[p] = rewards[p];
      st_perts[p] = perturbations[p];
    }
    if (tid == 0) st_best = best_reward[0];
    if (w_staged) {
      for (int e = tid; e < n_scal * M; e += SWEEP_THREADS) {
        w_lds[e] = weights[e];
      }
    }
    __syncthreads();
  }

  for (long long it = it_start; it < it_start + iterations; ++it) {
    const unsigned long long offset = (unsigned long long)it;
    // Parity slot of this iteration: candidates, M mean sums, distance.
    float* slot_c = slot_ws + (long)(it & 1) * batch_size * (dc + M + 1);
    float* slot_mu = slot_c + batch_size * dc;
    float* slot_dist = slot_mu + M * batch_size;
    const int batch_start =
        (int)(offset % (unsigned long long)n_batches) * batch_size;
    if (profwg) tmark = wall_clock64();

    // ---- Phase A: suggest (eagle_sweep.hip's, resident) + M k-vectors ----
    for (int b = blockIdx.x; b < batch_size; b += G) {
      const int me = batch_start + b;
      const float my_reward = st_rewards[me];
      const float my_pert = st_perts[me];
      for (int p = wt; p < pool_size; p += BLOCK) {
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
        const float reward_p = st_rewards[p];
        const float dir = (reward_p - my_reward >= 0.0f) ? gravity
                                                         : -neg_gravity;
        const float force = __expf(-visibility * d2 / dc * 10.0f);
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
      for (int j = wt; j < dc; j += BLOCK) {
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
        xq_lds[j] = cand;
      }
      __syncthreads();

      // The M k-vectors, mean sums and the distance of candidate b.
      float mu_acc[M];
#pragma unroll
      for (int m = 0; m < M; ++m) mu_acc[m] = 0.0f;
      float min_linf = INFINITY;
      if (x_vec4) {
        sweep_kvec_mo<M, true>(x, inv_ls, alpha, tr_mask, xq_lds,
                               k_ws + (long)b * n, k_stride, dc, n, wt, P,
                               mu_acc, min_linf);
      } else {
        sweep_kvec_mo<M, false>(x, inv_ls, alpha, tr_mask, xq_lds,
                                k_ws + (long)b * n, k_stride, dc, n, wt, P,
                                mu_acc, min_linf);
      }
      mo_block_reduce<M>(mu_acc, min_linf, red_mo);
      if (tid == 0) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
          mu_ws[m * batch_size + b] = mu_acc[m];
          cstore(slot_mu + m * batch_size + b, mu_acc[m]);
        }
        dist_ws[b] = min_linf;
        cstore(slot_dist + b, min_linf);
      }
      __syncthreads();
    }
    VZ_SWEEP_PROF(0)
    grid_sync(barrier_buf, bar_target);
    VZ_SWEEP_PROF(1)

    // ---- Phase B: M * T * T quadform items over the grid's halves ----
    {
      float* k_i_lds = half == 0 ? pool_lds : stage1_lds;
      float* k_j_lds = k_i_lds + VZ_QF_QMAX * VZ_QF_TILE;
      for (int item0 = blockIdx.x; item0 < total_items; item0 += 2 * G) {
        const int item = item0 + half * G;
        const bool live = item < total_items;
        // Metric and tile of the item; a half past the list keeps valid
        // values it does not use.
        const int m = live ? item / total_tiles : 0;
        const int t = live ? item - m * total_tiles : 0;
        const float* kinv_m = P.kinv[0];
#pragma unroll
        for (int mm = 1; mm < M; ++mm) kinv_m = (m == mm) ? P.kinv[mm] : kinv_m;
        const float* k_m = k_ws + m * k_stride;
        float* var_m = var_ws + m * var_stride;
        vz_quadform_tile_pipelined(
            kinv_m, batch_size, n, t, tiles_n, htid, live, k_i_lds, k_j_lds,
            [&](long idx) { return cload(k_m + idx); },
            [&](int q, float v) {
              cstore(var_m + (long)q * (total_tiles + 1) + t, v);
            },
            blockIdx.x == 0 ? iter_ptr + 10 : nullptr);
      }
    }
    VZ_SWEEP_PROF(2)
    grid_sync(barrier_buf, bar_target);
    VZ_SWEEP_PROF(3)

    // ---- RC: reduce + scalarise + update, on every owner ----
    // Scratch in phase B's staging area of half 0, free until the next B.
    float* wp = pool_lds;                                  // M x 4 x QMAX
    float* y_lds = wp + MO_MAX_M * 4 * VZ_QF_QMAX;         // M x QMAX
    float* sp = y_lds + MO_MAX_M * VZ_QF_QMAX;             // 4 x QMAX
    float* sc_lds = sp + 4 * VZ_QF_QMAX;                   // QMAX
    if (owner) {
      // 1. Tile partials of metric m, all candidates: half m & 1.
#pragma unroll
      for (int m0 = 0; m0 < M; m0 += 2) {
        const int m = m0 + half;
        if (m < M) {
          reduce_all_partials_at(var_ws + m * var_stride, batch_size,
                                 total_tiles, wp + m * 4 * VZ_QF_QMAX, htid);
        }
      }
      __syncthreads();
      // 2. mean, sd and the UCB term of every metric of candidate tid.
      if (tid < batch_size) {
        const bool publish = tid % G == (int)blockIdx.x;
#pragma unroll
        for (int m = 0; m < M; ++m) {
          const float quad = fold_quad(wp + m * 4 * VZ_QF_QMAX, tid);
          const float mean = cload(slot_mu + m * batch_size + tid) +
                             P.mean_c[m];
          const float sd = sqrtf(fmaxf(P.amp2[m] - quad, 1e-12f));
          float y = mean + coef * sd;
          if (ref) y -= ref[m];
          y_lds[m * VZ_QF_QMAX + tid] = y;
          if (publish) {
            var_ws[m * var_stride + (long)tid * (total_tiles + 1) +
                   total_tiles] = quad;
            ms_ws[m * batch_size + tid] = mean;
            ms_ws[(M + m) * batch_size + tid] = sd;
          }
        }
      }
      __syncthreads();
      // 3. Candidate c0 + half: hv_scalarize_tr_kernel's strided sum and
      // the shuffle tree of block_reduce; wave partials to sp.
      for (int c0 = 0; c0 < batch_size; c0 += 2) {
        const int c = c0 + half;
        const bool live = c < batch_size;
        const int cc = live ? c : batch_size - 1;
        float ym[M];
#pragma unroll
        for (int m = 0; m < M; ++m) ym[m] = y_lds[m * VZ_QF_QMAX + cc];
        float acc = 0.0f;
        for (int si = htid; si < n_scal; si += BLOCK) {
          float v = INFINITY;
#pragma unroll
          for (int m = 0; m < M; ++m) {
            v = fminf(v, ym[m] / wsrc[si * M + m]);
          }
          acc += v;
        }
        acc = wave_reduce_sum(acc);
        if (live && (tid & (WAVE_SIZE - 1)) == 0) {
          sp[(htid / WAVE_SIZE) * VZ_QF_QMAX + c] = acc;
        }
      }
      __syncthreads();
      // 4. Scores and the batch maximum (batch <= VZ_QF_QMAX < WAVE_SIZE).
      if (tid < WAVE_SIZE) {
        float score = -INFINITY;
        if (tid < batch_size) {
          const float total = fold_quad(sp, tid);
          score = total / (float)n_scal;
          const float dist = cload(slot_dist + tid);
          if (tr_radius > 0.0f && tr_radius <= 0.5f && dist > tr_radius) {
            score = -1e4f - dist;
          }
          sc_lds[tid] = score;
          if (tid % G == (int)blockIdx.x) score_ws[tid] = score;
        }
        const float batch_max = wave_reduce_max(score);
        if (tid == 0) s_scalar = fmaxf(st_best, batch_max);
      }
      __syncthreads();
      // 5. The update of all fireflies of the batch (eagle_sweep.hip, RC).
      const float new_best = s_scalar;
      for (int e = wt; e < batch_size * dc; e += BLOCK) {
        const int i = e / dc;
        const int me = batch_start + i;
        const int ej = me * dc + (e - i * dc);
        const float new_r = sc_lds[i];
        const float old_r = st_rewards[me];
        const bool improved = new_r > old_r;
        const float old_pert = st_perts[me];
        const float pert = improved ? old_pert : old_pert * penalize_factor;
        const float reward = improved ? new_r : old_r;
        const bool dead = (pert < perturbation_lower_bound) &&
                          (reward != new_best);
        if (dead) {
          st_pool[ej] = vz_rng_uniform<float>(
              seed_update, offset ^ 0x5151ull, (unsigned)ej);
        } else if (improved) {
          st_pool[ej] = cload(slot_c + e);
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
#undef VZ_SWEEP_PROF

  // Every owner holds the same final state; workgroup 0 hands it back.
  if (blockIdx.x == 0 && iterations > 0) {
    for (int e = wt; e < pool_elems; e += BLOCK) {
      cstore(pool_cont + e, st_pool[e]);
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

namespace {

// Cooperative launch of one instantiation with an occupancy-clamped grid,
// as launch_eagle_sweep (see there for the ordinary-launch fall-back when
// the device's cooperative queue belongs to another process).
template <int M>
int launch_mo(void** args, int n, hipStream_t stream) {
  const void* kernel = (const void*)eagle_sweep_mo_kernel<M>;
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
      &blocks_per_cu, kernel, SWEEP_THREADS, 0);
  if (err != hipSuccess || blocks_per_cu < 1) return 0;
  // The item list of phase B is M times eagle_sweep.hip's tile list; the
  // cap of 128 workgroups (the arrivals at the barrier) and the floor of
  // 64 (phase A at small N) are the same. VIZIER_AMD_SWEEP_GRID is read on
  // every call.
  const int tiles_n = (n + VZ_QF_TILE - 1) / VZ_QF_TILE;
  int grid = M * tiles_n * tiles_n;
  if (grid > 128) grid = 128;
  if (grid < 64) grid = 64;
  const char* env = getenv("VIZIER_AMD_SWEEP_GRID");
  const int grid_env = (env != nullptr) ? atoi(env) : 0;
  if (grid_env > 0) grid = grid_env;
  const int max_grid = blocks_per_cu * num_cu;
  if (grid > max_grid) grid = max_grid;
  if (grid < 1) grid = 1;
  err = hipLaunchCooperativeKernel(kernel, dim3(grid), dim3(SWEEP_THREADS),
                                   args, 0, stream);
  if (err == hipErrorIllegalState) {
    (void)hipGetLastError();  // handled here: leave none for a later check
    err = hipLaunchKernel(kernel, dim3(grid), dim3(SWEEP_THREADS), args, 0,
                          stream);
  }
  if (err != hipSuccess) return -(int)err;
  return grid;
}

}  // namespace

// Returns the grid size used, 0 if cooperative launch is unavailable, or a
// negative hipError_t on failure. 2 <= m <= MO_MAX_M is the caller's check.
extern "C" int launch_eagle_sweep_mo(
    float* pool_cont, float* rewards, float* perturbations,
    float* best_reward, unsigned long long* iter_ptr,
    unsigned int* barrier_buf, const float* x, const float* inv_ls,
    const float* alpha, const float* const* kinv, const float* amp2,
    const float* mean_c, const float* weights, const float* ref,
    const unsigned char* tr_mask, float* out_cont, float* k_ws, float* mu_ws,
    float* dist_ws, float* var_ws, float* ms_ws, float* score_ws,
    float* slot_ws, int m, int n_batches, int batch_size, int pool_size,
    int dc, int n, int n_scal, long long it_start, long long iterations,
    float visibility, float gravity, float neg_gravity, float norm_scale,
    float penalize_factor, float perturbation_lower_bound,
    float base_perturbation, unsigned long long seed_suggest,
    unsigned long long seed_update, float coef, float tr_radius,
    hipStream_t stream) {
  MoMetrics P;
  for (int i = 0; i < MO_MAX_M; ++i) {
    const int s = i < m ? i : m - 1;
    P.kinv[i] = kinv[s];
    P.amp2[i] = amp2[s];
    P.mean_c[i] = mean_c[s];
  }
  void* args[] = {
      &pool_cont, &rewards, &perturbations, &best_reward, &iter_ptr,
      &barrier_buf, &x, &inv_ls, &alpha, &P, &weights, &ref, &tr_mask,
      &out_cont, &k_ws, &mu_ws, &dist_ws, &var_ws, &ms_ws, &score_ws,
      &slot_ws, &n_batches, &batch_size, &pool_size, &dc, &n, &n_scal,
      &it_start, &iterations, &visibility, &gravity, &neg_gravity,
      &norm_scale, &penalize_factor, &perturbation_lower_bound,
      &base_perturbation, &seed_suggest, &seed_update, &coef, &tr_radius};
  switch (m) {
    case 2: return launch_mo<2>(args, n, stream);
    case 3: return launch_mo<3>(args, n, stream);
    case 4: return launch_mo<4>(args, n, stream);
    default: return -(int)hipErrorInvalidValue;
  }
}
