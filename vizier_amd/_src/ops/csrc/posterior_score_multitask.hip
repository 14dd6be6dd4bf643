// Fused posterior scorer for the separable multitask GP (gfx950).
//
// Numeric spec: multitask.MultitaskFusedCache. The joint covariance is
// K = Kx (x) B + tau I with Kx the unit-amplitude Matern-5/2 Gram and B the
// M x M task covariance. With B = U diag(lambda) U^T the joint system splits
// into M independent N x N systems W_s = (lambda_s Kx + tau I)^-1:
//   k[n]    = m52(|(xq - x_n)/ls|)                 (shared by all tasks)
//   quad_s  = k^T W_s k                            s = 0..M-1
//   var_t   = max(B_tt - sum_s c[t,s] quad_s, 1e-12),  c[t,s] = lambda_s^2 U[t,s]^2
//   mean_t  = means_t + k . a_mat[:, t],           a_mat = alpha_mat B
//   dist    = min_n max_{d not one-hot} |xq_d - x_nd|
// so one k-vector and M quadforms against N x N matrices replace the
// (NM) x (NM) triangular solve of MultitaskPosterior.predict.
//
// Three kernels, no atomics, every sum in one fixed order:
//  - mt_kvec_kernel: a workgroup owns a 64-row tile of the training set
//    (transposed through LDS in 64-column chunks, lane = row, as
//    posterior_score_linear.hip does) and serves a group of 32 candidates.
//    All M mean partials ride on that one pass over X.
//  - mt_quadform_kernel: work items are the upper-triangular pairs of 64 x 64
//    tiles (ti <= tj); every W_s is symmetric (the cache symmetrises it
//    exactly), so an off-diagonal item counts twice and each W_s is read half
//    as often as a full sweep would. The k_i and k_j slabs of the 32
//    candidates are staged in LDS once per item and reused for all M
//    matrices. Wave w owns candidates 8w..8w+7, lane = tile column, so a row
//    of the W_s tile is one coalesced 256-byte read. The tile streams through
//    two 32-row register buffers: the loads of the next half tile (of the
//    next s at the end of a tile) are issued before the FMAs of the current
//    one.
//  - mt_finalize_kernel: one wave per candidate sums the partials (lane-
//    strided, then a shuffle tree) and writes means (M, b), sds (M, b) and
//    dist (b), the layout hv_scalarize_tr consumes.
// gfx950 has no fp32 MFMA (see posterior_score.hip) and the quadforms are
// subtracted from B_tt, so everything stays fp32 on the vector ALU.

#include <hip/hip_runtime.h>
#include "common.h"
#include "mt_tile.h"

#define MT_MMAX 8      // tasks

extern "C" __global__ __launch_bounds__(MT_BLOCK) MT_NOPK void
mt_kvec_kernel(const float* __restrict__ xq,      // (B, D)
               const float* __restrict__ x,       // (N, D)
               const float* __restrict__ inv_ls,  // (D,)
               const float* __restrict__ a_mat,   // (N, M)
               const unsigned char* __restrict__ onehot,  // (D,)
               float* __restrict__ k_out,      // (B, N)
               float* __restrict__ mu_part,    // (B, M, tiles)
               float* __restrict__ dist_part,  // (B, tiles)
               int b, int n, int d, int m) {
  __shared__ float x_t[MT_COLS * MT_LD];
  __shared__ __attribute__((aligned(16))) float xq_s[MT_COLS * MT_Q];

  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  const int tiles = gridDim.x;
  const int tile = blockIdx.x;
  const int row0 = tile * MT_ROWS;
  const int q0 = blockIdx.y * MT_Q;
  const int row = row0 + lane;
  const bool row_ok = row < n;

  float d2[MT_QW], linf[MT_QW];
#pragma unroll
  for (int qq = 0; qq < MT_QW; ++qq) {
    d2[qq] = 0.0f;
    linf[qq] = 0.0f;
  }

  for (int c0 = 0; c0 < d; c0 += MT_COLS) {
    const int clen = min(MT_COLS, d - c0);
    // Stage the x tile: e runs along the row-major source. Rows past n
    // read as zeros; their results are masked below.
    for (int e = tid; e < MT_ROWS * clen; e += MT_BLOCK) {
      const int r = e / clen, c = e - r * clen;
      const int rr = row0 + r;
      x_t[c * MT_LD + r] = rr < n ? x[(long)rr * d + c0 + c] : 0.0f;
    }
    // Stage the candidate group; wave w's candidates w, w + 4, ... sit side
    // by side. Candidates past b are zeros and never written back.
    for (int e = tid; e < MT_Q * clen; e += MT_BLOCK) {
      const int ql = e / clen, c = e - ql * clen;
      const int q = q0 + ql;
      const int slot = (ql % MT_WAVES) * MT_QW + ql / MT_WAVES;
      xq_s[c * MT_Q + slot] = q < b ? xq[(long)q * d + c0 + c] : 0.0f;
    }
    __syncthreads();

#pragma unroll 2
    for (int c = 0; c < clen; ++c) {
      const float xv = x_t[c * MT_LD + lane];
      const float il = inv_ls[c0 + c];        // uniform: scalar load
      const bool cont = onehot[c0 + c] == 0;  // uniform branch
      const float4* xq4 =
          reinterpret_cast<const float4*>(&xq_s[c * MT_Q + wave * MT_QW]);
      const float4 xa = xq4[0], xb = xq4[1];
      const float xqv[MT_QW] = {xa.x, xa.y, xa.z, xa.w,
                                xb.x, xb.y, xb.z, xb.w};
#pragma unroll
      for (int qq = 0; qq < MT_QW; ++qq) {
        const float diff = xqv[qq] - xv;
        const float t = diff * il;
        d2[qq] = fmaf(t, t, d2[qq]);
        if (cont) linf[qq] = fmaxf(linf[qq], fabsf(diff));
      }
    }
    __syncthreads();
  }

  float a[MT_MMAX];
#pragma unroll
  for (int t = 0; t < MT_MMAX; ++t) {
    a[t] = (row_ok && t < m) ? a_mat[(long)row * m + t] : 0.0f;
  }
#pragma unroll
  for (int qq = 0; qq < MT_QW; ++qq) {
    const int q = q0 + wave + qq * MT_WAVES;  // wave-uniform
    const float kv = row_ok ? matern52_of_d2(d2[qq]) : 0.0f;
    if (row_ok && q < b) k_out[(long)q * n + row] = kv;
    const float dist = wave_reduce_min(row_ok ? linf[qq] : INFINITY);
    if (lane == 0 && q < b) dist_part[(long)q * tiles + tile] = dist;
#pragma unroll
    for (int t = 0; t < MT_MMAX; ++t) {
      if (t < m) {  // uniform
        const float mu = wave_reduce_sum(kv * a[t]);
        if (lane == 0 && q < b) {
          mu_part[((long)q * m + t) * tiles + tile] = mu;
        }
      }
    }
  }
}

extern "C" __global__ __launch_bounds__(MT_BLOCK) MT_NOPK void
mt_quadform_kernel(const float* __restrict__ k,  // (B, N)
                   const float* __restrict__ w,  // (M, N, N), symmetric
                   float* __restrict__ part,     // (B, M, items)
                   int b, int n, int m, int tiles_n, int items) {
  __shared__ __attribute__((aligned(16))) float ki_s[MT_ROWS * MT_KLD];
  __shared__ float kj_s[MT_Q * MT_ROWS];

  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  const int q0 = blockIdx.y * MT_Q;

  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    // item -> (ti, tj), row-major over the upper triangle.
    int ti = 0, rem = item;
    while (rem >= tiles_n - ti) {
      rem -= tiles_n - ti;
      ++ti;
    }
    const int tj = ti + rem;
    const int i0 = ti * MT_ROWS, j0 = tj * MT_ROWS;

    for (int e = tid; e < MT_Q * MT_ROWS; e += MT_BLOCK) {
      const int ql = e / MT_ROWS, c = e % MT_ROWS;
      const int q = q0 + ql;
      const float* kq = k + (long)q * n;
      ki_s[c * MT_KLD + ql] = (q < b && i0 + c < n) ? kq[i0 + c] : 0.0f;
      kj_s[e] = (q < b && j0 + c < n) ? kq[j0 + c] : 0.0f;
    }
    __syncthreads();

    const int col = j0 + lane;
    const float weight = ti == tj ? 1.0f : 2.0f;
    float wa[MT_HALF], wb[MT_HALF];
    mt_load_half(wa, w, i0, col, n);
    for (int s = 0; s < m; ++s) {
      const float* ws = w + (long)s * n * n;
      float acc[MT_QW];
#pragma unroll
      for (int qq = 0; qq < MT_QW; ++qq) acc[qq] = 0.0f;
      // The k_i slab does not change with s, so its 128 LDS reads (512
      // registers) get hoisted out of this loop and spilled. At an offset
      // the compiler cannot see through they stay where they are.
      int ko = wave * MT_QW;
      __asm__ volatile("" : "+v"(ko));
      const float* ki_w = ki_s + ko;
      mt_load_half(wb, ws, i0 + MT_HALF, col, n);
      mt_fma_half(acc, wa, ki_w);
      // Pin the FMAs here: otherwise they sink below the branch that
      // refills wa, and the LDS reads that feed them are spilled meanwhile.
      __asm__ volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]),
                            "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]),
                            "+v"(acc[6]), "+v"(acc[7]));
      if (s + 1 < m) mt_load_half(wa, ws + (long)n * n, i0, col, n);
      mt_fma_half(acc, wb, ki_w + MT_HALF * MT_KLD);
      __asm__ volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]),
                            "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]),
                            "+v"(acc[6]), "+v"(acc[7]));
#pragma unroll
      for (int qq = 0; qq < MT_QW; ++qq) {
        const int ql = wave * MT_QW + qq;
        const float v =
            wave_reduce_sum(acc[qq] * kj_s[ql * MT_ROWS + lane]);
        if (lane == 0 && q0 + ql < b) {
          part[((long)(q0 + ql) * m + s) * items + item] = weight * v;
        }
      }
    }
    __syncthreads();  // the slabs are restaged on the next trip
  }
}

// One wave per candidate. Lane l sums partials l, l + 64, ... in index
// order, then a shuffle tree: one fixed order, identical from run to run.
extern "C" __global__ __launch_bounds__(WAVE_SIZE) MT_NOPK void
mt_finalize_kernel(const float* __restrict__ part,       // (B, M, items)
                   const float* __restrict__ mu_part,    // (B, M, tiles)
                   const float* __restrict__ dist_part,  // (B, tiles)
                   const float* __restrict__ c,          // (M, M)
                   const float* __restrict__ bdiag,      // (M,)
                   const float* __restrict__ means,      // (M,)
                   float* __restrict__ mean_out,         // (M, B)
                   float* __restrict__ sd_out,           // (M, B)
                   float* __restrict__ dist_out,         // (B,)
                   int b, int m, int tiles, int items) {
  const int q = blockIdx.x;
  const int lane = threadIdx.x;
  float quad[MT_MMAX], mu[MT_MMAX];
#pragma unroll
  for (int s = 0; s < MT_MMAX; ++s) {
    quad[s] = 0.0f;
    mu[s] = 0.0f;
    if (s < m) {  // uniform
      const float* pp = part + ((long)q * m + s) * items;
      const float* mp = mu_part + ((long)q * m + s) * tiles;
      float v = 0.0f, u = 0.0f;
      for (int i = lane; i < items; i += WAVE_SIZE) v += pp[i];
      for (int i = lane; i < tiles; i += WAVE_SIZE) u += mp[i];
      quad[s] = wave_reduce_sum(v);
      mu[s] = wave_reduce_sum(u);
    }
  }
  float dist = INFINITY;
  for (int i = lane; i < tiles; i += WAVE_SIZE) {
    dist = fminf(dist, dist_part[(long)q * tiles + i]);
  }
  dist = wave_reduce_min(dist);
  if (lane != 0) return;
  dist_out[q] = dist;
#pragma unroll
  for (int t = 0; t < MT_MMAX; ++t) {
    if (t < m) {
      float red = 0.0f;
#pragma unroll
      for (int s = 0; s < MT_MMAX; ++s) {
        if (s < m) red = fmaf(c[t * m + s], quad[s], red);
      }
      mean_out[(long)t * b + q] = means[t] + mu[t];
      sd_out[(long)t * b + q] = sqrtf(fmaxf(bdiag[t] - red, 1e-12f));
    }
  }
}

extern "C" int mt_num_tiles(int n) { return (n + MT_ROWS - 1) / MT_ROWS; }

extern "C" int mt_num_items(int n) {
  const int t = mt_num_tiles(n);
  return t * (t + 1) / 2;
}

extern "C" void launch_mt_mean_std(
    const float* xq, const float* x, const float* inv_ls, const float* a_mat,
    const float* w, const float* c, const float* bdiag, const float* means,
    const unsigned char* onehot, float* k_ws, float* part, float* mu_part,
    float* dist_part, float* mean_out, float* sd_out, float* dist_out, int b,
    int n, int d, int m, hipStream_t stream) {
  const int tiles = mt_num_tiles(n), items = mt_num_items(n);
  const int groups = (b + MT_Q - 1) / MT_Q;
  hipLaunchKernelGGL(mt_kvec_kernel, dim3(tiles, groups), dim3(MT_BLOCK), 0,
                     stream, xq, x, inv_ls, a_mat, onehot, k_ws, mu_part,
                     dist_part, b, n, d, m);
  hipLaunchKernelGGL(mt_quadform_kernel,
                     dim3(items < MT_GRID_MAX ? items : MT_GRID_MAX, groups),
                     dim3(MT_BLOCK), 0,
                     stream, k_ws, w, part, b, n, m, tiles, items);
  hipLaunchKernelGGL(mt_finalize_kernel, dim3(b), dim3(WAVE_SIZE), 0, stream,
                     part, mu_part, dist_part, c, bdiag, means, mean_out,
                     sd_out, dist_out, b, m, tiles, items);
}
