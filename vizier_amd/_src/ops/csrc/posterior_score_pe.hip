// Fused scorer of GP-UCB-PE's single-point sweeps conditioned on pending
// points (gfx950): the UCB member with a trust region anchored on completed +
// pending rows, and the pure-exploration (PE) member.
//
// Numeric spec. x_all (Na, D) holds the fitted posterior's n_fit training rows
// first, then the pending / already chosen rows. With ls (D), amp, mean_c,
// alpha (n_fit), W_fit (n_fit, n_fit) = K_fit^-1 and, in PE mode, W_all
// (Na, Na) = K_all^-1:
//   k[i]    = amp^2 m52(|(xq - x_all[i]) / ls|)                   i < Na
//   mean    = mean_c + sum_{i < n_fit} k[i] alpha[i]
//   var     = max(amp^2 - k[:n_fit]^T W_fit k[:n_fit], 1e-12)
//   var_all = max(amp^2 - k^T W_all k, 1e-12)                     (PE only)
//   dist    = min_{i < Na} max_{d not one-hot} |xq_d - x_all[i, d]|
//   UCB: s = mean + c sd
//   PE:  s = sd_all + pen * min(mean + c_explore sd - thr, 0)
//   score = vz_trust_region(s, dist, tr_radius)
// Both posteriors share the hyperparameters and x_all[:n_fit] is the fitted
// x, so ONE k-vector serves both: the fitted posterior's is its first n_fit
// entries, bit for bit.
//
// CONTRACT: W_fit and W_all must be EXACTLY symmetric. The quadform reads only
// the tile pairs ti <= tj and counts the off-diagonal ones twice.
//
// Three kernels, no atomics, every sum in one fixed order:
//  - pe_kvec_kernel: a workgroup owns a 64-row tile of x_all and up to 32
//    candidates. The tile goes transposed through LDS in 64-column chunks
//    (lane = row); one pass gives k (row stride Na), the tile's L-inf partial
//    over ALL its rows and its mean partial, to which rows >= n_fit add an
//    exact 0 (their alpha reads as 0): the tile that straddles n_fit and the
//    tiles wholly past it need no case of their own.
//  - pe_quadform_kernel: the upper-triangular 64 x 64 tile pairs of W_fit,
//    then those of W_all, form one item list walked with a capped grid
//    stride. Both matrices read the same k buffer; a W_fit item masks the
//    columns >= n_fit of its slabs, where k holds the pending rows' values.
//    Per item the k_i / k_j slabs of the 32 candidates sit in LDS and the W
//    tile streams through two 32-row register buffers (mt_tile.h).
//  - pe_finalize_kernel: one wave per candidate; lane-strided sums of the
//    partials in index order, a shuffle tree, then the formulas above.
// gfx950 has no fp32 MFMA and both quadforms are subtracted from amp^2, so
// everything stays fp32 on the vector ALU.

#include <hip/hip_runtime.h>
#include "common.h"
#include "mt_tile.h"

#define PE_MODE_UCB 0
#define PE_MODE_PE 1

static int pe_tiles(int n) { return (n + MT_ROWS - 1) / MT_ROWS; }
static int pe_items(int n) { return pe_tiles(n) * (pe_tiles(n) + 1) / 2; }

extern "C" __global__ __launch_bounds__(MT_BLOCK) MT_NOPK void
pe_kvec_kernel(const float* __restrict__ xq,              // (B, D)
               const float* __restrict__ x,               // (Na, D)
               const float* __restrict__ inv_ls,          // (D,)
               const float* __restrict__ alpha,           // (n_fit,)
               const unsigned char* __restrict__ onehot,  // (D,)
               float* __restrict__ k_out,                 // (B, Na)
               float* __restrict__ mu_part,               // (B, tiles)
               float* __restrict__ dist_part,             // (B, tiles)
               int b, int na, int n_fit, int d, float amp2) {
  __shared__ float x_t[MT_COLS * MT_LD];
  __shared__ __attribute__((aligned(16))) float xq_s[MT_COLS * MT_Q];
  __shared__ float ils_s[MT_COLS];  // the chunk's 1/ls
  __shared__ int cont_s[MT_COLS];   // the chunk's columns that enter dist

  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  const int tile = blockIdx.x, tiles = gridDim.x;
  const int row0 = tile * MT_ROWS;
  const int q0 = blockIdx.y * MT_Q;
  const int row = row0 + lane;
  const bool row_ok = row < na;

  float d2[MT_QW], linf[MT_QW];
#pragma unroll
  for (int qq = 0; qq < MT_QW; ++qq) {
    d2[qq] = 0.0f;
    linf[qq] = 0.0f;
  }

  for (int c0 = 0; c0 < d; c0 += MT_COLS) {
    const int clen = min(MT_COLS, d - c0);
    // Rows past Na read as zeros; their results are masked below.
    for (int e = tid; e < MT_ROWS * clen; e += MT_BLOCK) {
      const int r = e / clen, c = e - r * clen;
      const int rr = row0 + r;
      x_t[c * MT_LD + r] = rr < na ? x[(long)rr * d + c0 + c] : 0.0f;
    }
    // Wave w's candidates w, w + 4, ... sit side by side. Candidates past b
    // are zeros and never written back.
    for (int e = tid; e < MT_Q * clen; e += MT_BLOCK) {
      const int ql = e / clen, c = e - ql * clen;
      const int q = q0 + ql;
      const int slot = (ql % MT_WAVES) * MT_QW + ql / MT_WAVES;
      xq_s[c * MT_Q + slot] = q < b ? xq[(long)q * d + c0 + c] : 0.0f;
    }
    if (tid < clen) {
      ils_s[tid] = inv_ls[c0 + tid];
      cont_s[tid] = onehot[c0 + tid] == 0;
    }
    __syncthreads();

    for (int c = 0; c < clen; ++c) {
      const float xv = x_t[c * MT_LD + lane];
      const float s = ils_s[c];  // broadcast reads
      const float4* xq4 =
          reinterpret_cast<const float4*>(&xq_s[c * MT_Q + wave * MT_QW]);
      const float4 xa = xq4[0], xb = xq4[1];
      const float diff[MT_QW] = {xa.x - xv, xa.y - xv, xa.z - xv, xa.w - xv,
                                 xb.x - xv, xb.y - xv, xb.z - xv, xb.w - xv};
      if (cont_s[c]) {  // uniform
#pragma unroll
        for (int qq = 0; qq < MT_QW; ++qq) {
          linf[qq] = fmaxf(linf[qq], fabsf(diff[qq]));
        }
      }
#pragma unroll
      for (int qq = 0; qq < MT_QW; ++qq) {
        const float t = diff[qq] * s;
        d2[qq] = fmaf(t, t, d2[qq]);
      }
    }
    __syncthreads();
  }

  const float al = row < n_fit ? alpha[row] : 0.0f;
#pragma unroll
  for (int qq = 0; qq < MT_QW; ++qq) {
    const int q = q0 + wave + qq * MT_WAVES;  // wave-uniform
    const float kv = row_ok ? amp2 * matern52_of_d2(d2[qq]) : 0.0f;
    if (row_ok && q < b) k_out[(long)q * na + row] = kv;
    const float mu = wave_reduce_sum(kv * al);
    const float dist = wave_reduce_min(row_ok ? linf[qq] : INFINITY);
    if (lane == 0 && q < b) {
      mu_part[(long)q * tiles + tile] = mu;
      dist_part[(long)q * tiles + tile] = dist;
    }
  }
}

// Items [0, items_fit) are W_fit's tile pairs, [items_fit, items) W_all's.
extern "C" __global__ __launch_bounds__(MT_BLOCK) MT_NOPK void
pe_quadform_kernel(const float* __restrict__ k,      // (B, Na)
                   const float* __restrict__ w_fit,  // (n_fit, n_fit)
                   const float* __restrict__ w_all,  // (Na, Na) or NULL
                   float* __restrict__ part,         // (B, items)
                   int b, int na, int n_fit, int items_fit, int items) {
  __shared__ __attribute__((aligned(16))) float ki_s[MT_ROWS * MT_KLD];
  __shared__ float kj_s[MT_Q * MT_ROWS];

  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  const int q0 = blockIdx.y * MT_Q;

  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const bool fit = item < items_fit;  // uniform
    const int n = fit ? n_fit : na;
    const float* __restrict__ w = fit ? w_fit : w_all;
    const int tiles_n = (n + MT_ROWS - 1) / MT_ROWS;
    // item -> (ti, tj), row-major over the matrix's upper triangle.
    int ti = 0, rem = fit ? item : item - items_fit;
    while (rem >= tiles_n - ti) {
      rem -= tiles_n - ti;
      ++ti;
    }
    const int tj = ti + rem;
    const int i0 = ti * MT_ROWS, j0 = tj * MT_ROWS;

    // Entries at or past n read as zeros: past Na there is nothing, and for
    // W_fit the entries n_fit .. Na - 1 belong to the pending rows.
    for (int e = tid; e < MT_Q * MT_ROWS; e += MT_BLOCK) {
      const int ql = e / MT_ROWS, c = e % MT_ROWS;
      const int q = q0 + ql;
      const float* kq = k + (long)q * na;
      ki_s[c * MT_KLD + ql] = (q < b && i0 + c < n) ? kq[i0 + c] : 0.0f;
      kj_s[e] = (q < b && j0 + c < n) ? kq[j0 + c] : 0.0f;
    }
    __syncthreads();

    const int col = j0 + lane;
    const float weight = ti == tj ? 1.0f : 2.0f;
    float wa[MT_HALF], wb[MT_HALF], acc[MT_QW];
#pragma unroll
    for (int qq = 0; qq < MT_QW; ++qq) acc[qq] = 0.0f;
    // An offset the compiler cannot see through: otherwise the k_i slab's
    // 128 LDS reads are all issued up front and held in registers.
    int ko = wave * MT_QW;
    __asm__ volatile("" : "+v"(ko));
    const float* ki_w = ki_s + ko;
    mt_load_half(wa, w, i0, col, n);
    mt_load_half(wb, w, i0 + MT_HALF, col, n);
    mt_fma_half(acc, wa, ki_w);
    // Pin the FMAs here, ahead of the second half's LDS reads.
    __asm__ volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]),
                          "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]),
                          "+v"(acc[6]), "+v"(acc[7]));
    mt_fma_half(acc, wb, ki_w + MT_HALF * MT_KLD);
    __asm__ volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]),
                          "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]),
                          "+v"(acc[6]), "+v"(acc[7]));
#pragma unroll
    for (int qq = 0; qq < MT_QW; ++qq) {
      const int ql = wave * MT_QW + qq;
      const float v = wave_reduce_sum(acc[qq] * kj_s[ql * MT_ROWS + lane]);
      if (lane == 0 && q0 + ql < b) {
        part[(long)(q0 + ql) * items + item] = weight * v;
      }
    }
    __syncthreads();  // the slabs are restaged on the next trip
  }
}

// Lane l sums entries l, l + 64, ... of [lo, hi) in index order, then a
// shuffle tree: one fixed order, identical from run to run.
__device__ __forceinline__ float pe_sum_range(const float* __restrict__ p,
                                              int lo, int hi, int lane) {
  float v = 0.0f;
  for (int i = lo + lane; i < hi; i += WAVE_SIZE) v += p[i];
  return wave_reduce_sum(v);
}

// One wave per candidate. score != NULL writes the score alone; otherwise
// (mean, sd, dist) and, in PE mode, sd_all.
extern "C" __global__ __launch_bounds__(WAVE_SIZE) MT_NOPK void
pe_finalize_kernel(const float* __restrict__ part,       // (B, items)
                   const float* __restrict__ mu_part,    // (B, tiles)
                   const float* __restrict__ dist_part,  // (B, tiles)
                   float* __restrict__ score, float* __restrict__ mean_out,
                   float* __restrict__ sd_out, float* __restrict__ sd_all_out,
                   float* __restrict__ dist_out, int tiles, int items_fit,
                   int items, float amp2, float mean_c, int mode, float coef,
                   float explore_coef, float threshold, float pen_coef,
                   float tr_radius) {
  const int q = blockIdx.x;
  const int lane = threadIdx.x;
  const float* pp = part + (long)q * items;
  const float quad = pe_sum_range(pp, 0, items_fit, lane);
  const float quad_all = pe_sum_range(pp, items_fit, items, lane);
  const float mu = pe_sum_range(mu_part + (long)q * tiles, 0, tiles, lane);
  float dist = INFINITY;
  for (int i = lane; i < tiles; i += WAVE_SIZE) {
    dist = fminf(dist, dist_part[(long)q * tiles + i]);
  }
  dist = wave_reduce_min(dist);
  if (lane != 0) return;

  const float mean = mean_c + mu;
  const float sd = sqrtf(fmaxf(amp2 - quad, 1e-12f));
  const float sd_all = sqrtf(fmaxf(amp2 - quad_all, 1e-12f));
  if (score != nullptr) {
    float s;
    if (mode == PE_MODE_PE) {
      const float explore = fmaf(explore_coef, sd, mean);
      s = fmaf(pen_coef, fminf(explore - threshold, 0.0f), sd_all);
    } else {
      s = vz_acq_score(ACQ_UCB, mean, sd, coef, 0.0f);
    }
    score[q] = vz_trust_region(s, dist, tr_radius);
  } else {
    mean_out[q] = mean;
    sd_out[q] = sd;
    dist_out[q] = dist;
    if (mode == PE_MODE_PE) sd_all_out[q] = sd_all;
  }
}

// Workspace extents: 64-row tiles of x_all, W_fit's items, all items.
extern "C" void pe_layout(int na, int n_fit, int with_all, int* tiles,
                          int* items_fit, int* items) {
  *tiles = pe_tiles(na);
  *items_fit = pe_items(n_fit);
  *items = *items_fit + (with_all ? pe_items(na) : 0);
}

// w_all == NULL is UCB mode: its items do not exist. score != NULL: scores
// (b,); otherwise mean_out, sd_out, dist_out and (PE) sd_all_out (b,). The
// caller has checked every shape.
extern "C" void launch_pe(
    const float* xq, const float* x, const float* inv_ls, const float* alpha,
    const float* w_fit, const float* w_all, const unsigned char* onehot,
    float* k_ws, float* part, float* mu_part, float* dist_part, float* score,
    float* mean_out, float* sd_out, float* sd_all_out, float* dist_out, int b,
    int na, int n_fit, int d, float amp2, float mean_c, float coef,
    float explore_coef, float threshold, float pen_coef, float tr_radius,
    hipStream_t stream) {
  int tiles, items_fit, items;
  pe_layout(na, n_fit, w_all != nullptr, &tiles, &items_fit, &items);
  const int mode = w_all != nullptr ? PE_MODE_PE : PE_MODE_UCB;
  const int groups = (b + MT_Q - 1) / MT_Q;
  hipLaunchKernelGGL(pe_kvec_kernel, dim3(tiles, groups), dim3(MT_BLOCK), 0,
                     stream, xq, x, inv_ls, alpha, onehot, k_ws, mu_part,
                     dist_part, b, na, n_fit, d, amp2);
  hipLaunchKernelGGL(pe_quadform_kernel,
                     dim3(items < MT_GRID_MAX ? items : MT_GRID_MAX, groups),
                     dim3(MT_BLOCK), 0, stream, k_ws, w_fit, w_all, part, b,
                     na, n_fit, items_fit, items);
  hipLaunchKernelGGL(pe_finalize_kernel, dim3(b), dim3(WAVE_SIZE), 0, stream,
                     part, mu_part, dist_part, score, mean_out, sd_out,
                     sd_all_out, dist_out, tiles, items_fit, items, amp2,
                     mean_c, mode, coef, explore_coef, threshold, pen_coef,
                     tr_radius);
}
