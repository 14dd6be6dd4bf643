// Fused posterior scorer for the Matern-5/2 + linear kernel GP (gfx950).
//
// Numeric spec: linear_matern._combined_gram + LinearMaternPosterior.predict
// with s' = linear_coef * slope, c' = linear_coef * shift:
//   z_nd  = x_nd / ls_d - c'         zq_d = xq_d / ls_d - c'   (all D columns)
//   k[n]  = amp^2 m52(|(xq - x_n)/ls|) + s'^2 sum_d zq_d z_nd
//   mu    = mean + k . alpha
//   var   = max(amp^2 + s'^2 sum_d zq_d^2 - k^T Kinv k, 1e-12)
//   dist  = min_n max_{d not one-hot} |xq_d - x_nd|
//   score = trust_region(acq(mu, sqrt(var)), dist)
// Kinv is the inverse of the COMBINED kernel's Gram (K_inv_lin); the
// quadform between the two kernels here is the shared one of module.cpp.
//
// Work split (the reverse of ps_kvec_kernel, which gives a workgroup one
// candidate and lets every thread walk its own training row with stride D):
// a workgroup OWNS a 64-row tile of the training set and serves a group of
// up to 32 candidates from it.
//  - The tile goes through LDS in chunks of 64 columns, transposed to
//    [col][row] (row stride 65 floats): the global read runs along the
//    row-major source, the transposed writes fall in distinct banks, and
//    with lane = row every compute read of x is conflict-free.
//  - The candidates of the group sit in LDS as [col][slot], raw and scaled.
//    Wave w owns candidates w, w + 4, ... (8 of them); slot = (q % 4) * 8 +
//    q / 4 puts those 8 side by side, so a wave fetches them with two
//    128-bit reads at one address for all lanes (broadcast).
//  - One LDS read of an x element feeds 8 candidates x 3 accumulators (d2,
//    lin, linf) held in registers. Raw x is staged, not z: the trust-region
//    distance needs it, and z = fmaf(x, 1/ls, -c') is one FMA in registers.
//  - mu and dist leave as per-(candidate, tile) wave reductions in a partials
//    buffer, summed in tile order by the finalize kernel: no atomics, one
//    fixed order, identical results from run to run.
// gfx950 has no fp32 MFMA (see posterior_score.hip) and the linear term is
// subtracted against the quadform, so it stays fp32 on the vector ALU.

#include <hip/hip_runtime.h>
#include "common.h"

#define PSL_BLOCK 256
#define PSL_ROWS 64    // training rows per tile == WAVE_SIZE (lane = row)
#define PSL_COLS 64    // feature columns per LDS chunk
#define PSL_LD 65      // row stride of the transposed x tile
#define PSL_Q 32       // candidates per group
#define PSL_WAVES (PSL_BLOCK / WAVE_SIZE)
#define PSL_QW (PSL_Q / PSL_WAVES)  // candidates per wave

static_assert(PSL_ROWS == WAVE_SIZE, "lane = row");
static_assert(PSL_QW == 8, "two float4 reads per wave and column");

// Both kernels are compiled without packed fp32 instructions (v_pk_fma_f32
// and its kin), whatever flags the rest of the extension is built with.
extern "C" __global__ __launch_bounds__(PSL_BLOCK)
__attribute__((target("no-packed-fp32-ops"))) void
psl_kvec_tile_kernel(const float* __restrict__ xq,      // (B, D)
                     const float* __restrict__ x,       // (N, D)
                     const float* __restrict__ inv_ls,  // (D,)
                     const float* __restrict__ alpha,   // (N,)
                     const unsigned char* __restrict__ onehot,  // (D,)
                     float* __restrict__ k_out,      // (B, N)
                     float* __restrict__ mu_part,    // (B, tiles)
                     float* __restrict__ dist_part,  // (B, tiles)
                     float* __restrict__ zq2_out,    // (B,)
                     int b, int n, int d, float amp2, float s2,
                     float cshift) {
  __shared__ float x_t[PSL_COLS * PSL_LD];
  __shared__ __attribute__((aligned(16))) float xq_s[PSL_COLS * PSL_Q];
  __shared__ __attribute__((aligned(16))) float zq_s[PSL_COLS * PSL_Q];

  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  const int tiles = gridDim.x;
  const int tile = blockIdx.x;
  const int row0 = tile * PSL_ROWS;
  const int q0 = blockIdx.y * PSL_Q;
  const int row = row0 + lane;
  const bool row_ok = row < n;

  float d2[PSL_QW], lin[PSL_QW], linf[PSL_QW], zz[PSL_QW];
#pragma unroll
  for (int qq = 0; qq < PSL_QW; ++qq) {
    d2[qq] = 0.0f;
    lin[qq] = 0.0f;
    linf[qq] = 0.0f;
    zz[qq] = 0.0f;
  }

  for (int c0 = 0; c0 < d; c0 += PSL_COLS) {
    const int clen = min(PSL_COLS, d - c0);
    // Stage the x tile: e runs along the row-major source. Rows past n
    // read as zeros; their results are masked below.
    for (int e = tid; e < PSL_ROWS * clen; e += PSL_BLOCK) {
      const int r = e / clen, c = e - r * clen;
      const int rr = row0 + r;
      x_t[c * PSL_LD + r] = rr < n ? x[(long)rr * d + c0 + c] : 0.0f;
    }
    // Stage the candidate group, raw and scaled. Candidates past b are
    // zeros and never written back.
    for (int e = tid; e < PSL_Q * clen; e += PSL_BLOCK) {
      const int ql = e / clen, c = e - ql * clen;
      const int q = q0 + ql;
      const float v = q < b ? xq[(long)q * d + c0 + c] : 0.0f;
      const int slot = (ql % PSL_WAVES) * PSL_QW + ql / PSL_WAVES;
      xq_s[c * PSL_Q + slot] = v;
      zq_s[c * PSL_Q + slot] = fmaf(v, inv_ls[c0 + c], -cshift);
    }
    __syncthreads();

#pragma unroll 2
    for (int c = 0; c < clen; ++c) {
      const float xv = x_t[c * PSL_LD + lane];
      const float il = inv_ls[c0 + c];        // uniform: scalar load
      const bool cont = onehot[c0 + c] == 0;  // uniform branch
      const float zx = fmaf(xv, il, -cshift);
      const float4* xq4 =
          reinterpret_cast<const float4*>(&xq_s[c * PSL_Q + wave * PSL_QW]);
      const float4* zq4 =
          reinterpret_cast<const float4*>(&zq_s[c * PSL_Q + wave * PSL_QW]);
      const float4 xa = xq4[0], xb = xq4[1];
      const float4 za = zq4[0], zb = zq4[1];
      const float xqv[PSL_QW] = {xa.x, xa.y, xa.z, xa.w,
                                 xb.x, xb.y, xb.z, xb.w};
      const float zqv[PSL_QW] = {za.x, za.y, za.z, za.w,
                                 zb.x, zb.y, zb.z, zb.w};
#pragma unroll
      for (int qq = 0; qq < PSL_QW; ++qq) {
        const float diff = xqv[qq] - xv;
        const float t = diff * il;
        d2[qq] = fmaf(t, t, d2[qq]);
        lin[qq] = fmaf(zqv[qq], zx, lin[qq]);
        if (cont) linf[qq] = fmaxf(linf[qq], fabsf(diff));
      }
    }
    // |zq|^2 of the per-candidate prior: tile 0 only, lane = column.
    if (tile == 0 && lane < clen) {
#pragma unroll
      for (int qq = 0; qq < PSL_QW; ++qq) {
        const float z = zq_s[lane * PSL_Q + wave * PSL_QW + qq];
        zz[qq] = fmaf(z, z, zz[qq]);
      }
    }
    __syncthreads();
  }

  const float a = row_ok ? alpha[row] : 0.0f;
#pragma unroll
  for (int qq = 0; qq < PSL_QW; ++qq) {
    const int q = q0 + wave + qq * PSL_WAVES;
    const float kv = fmaf(s2, lin[qq], amp2 * matern52_of_d2(d2[qq]));
    const bool ok = row_ok && q < b;   // q is wave-uniform
    if (ok) k_out[(long)q * n + row] = kv;
    const float mu = wave_reduce_sum(row_ok ? kv * a : 0.0f);
    const float dist = wave_reduce_min(row_ok ? linf[qq] : INFINITY);
    const float z2 = tile == 0 ? wave_reduce_sum(zz[qq]) : 0.0f;
    if (lane == 0 && q < b) {
      mu_part[(long)q * tiles + tile] = mu;
      dist_part[(long)q * tiles + tile] = dist;
      if (tile == 0) zq2_out[q] = z2;
    }
  }
}

// One thread per candidate: the tile partials in index order, then the
// per-candidate prior, the acquisition and the trust region. score != NULL
// writes the score alone; otherwise (mean, sd, dist).
extern "C" __global__ __attribute__((target("no-packed-fp32-ops"))) void
psl_finalize_kernel(const float* __restrict__ mu_part,
                    const float* __restrict__ dist_part,
                    const float* __restrict__ zq2,
                    const float* __restrict__ quad,
                    float* __restrict__ score, float* __restrict__ mean_out,
                    float* __restrict__ sd_out, float* __restrict__ dist_out,
                    int b, int tiles, float amp2, float s2, float mean_c,
                    int acq, float coef, float best_value, float tr_radius) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= b) return;
  float mu = 0.0f, dist = INFINITY;
  const float* mp = mu_part + (long)q * tiles;
  const float* dp = dist_part + (long)q * tiles;
  int t = 0;
  // Eight loads of each array in flight at once; the sum keeps index order.
  for (; t + 8 <= tiles; t += 8) {
    float m[8], dd[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      m[u] = mp[t + u];
      dd[u] = dp[t + u];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      mu += m[u];
      dist = fminf(dist, dd[u]);
    }
  }
  for (; t < tiles; ++t) {
    mu += mp[t];
    dist = fminf(dist, dp[t]);
  }
  mu += mean_c;
  const float prior = fmaf(s2, zq2[q], amp2);
  const float sd = sqrtf(fmaxf(prior - quad[q], 1e-12f));
  if (score != nullptr) {
    score[q] = vz_trust_region(
        vz_acq_score(acq, mu, sd, coef, best_value), dist, tr_radius);
  } else {
    mean_out[q] = mu;
    sd_out[q] = sd;
    dist_out[q] = dist;
  }
}

extern "C" int psl_num_tiles(int n) {
  return (n + PSL_ROWS - 1) / PSL_ROWS;
}

extern "C" void launch_psl_kvec(
    const float* xq, const float* x, const float* inv_ls,
    const float* alpha, const unsigned char* onehot, float* k_ws,
    float* mu_part, float* dist_part, float* zq2, int b, int n, int d,
    float amp2, float s2, float cshift, hipStream_t stream) {
  const dim3 grid(psl_num_tiles(n), (b + PSL_Q - 1) / PSL_Q);
  hipLaunchKernelGGL(psl_kvec_tile_kernel, grid, dim3(PSL_BLOCK), 0, stream,
                     xq, x, inv_ls, alpha, onehot, k_ws, mu_part, dist_part,
                     zq2, b, n, d, amp2, s2, cshift);
}

extern "C" void launch_psl_finalize_score(
    const float* mu_part, const float* dist_part, const float* zq2,
    const float* quad, float* out, int b, int tiles, float amp2, float s2,
    float mean_c, int acq, float coef, float best_value, float tr_radius,
    hipStream_t stream) {
  const int block = 256;
  hipLaunchKernelGGL(psl_finalize_kernel, dim3((b + block - 1) / block),
                     dim3(block), 0, stream, mu_part, dist_part, zq2, quad,
                     out, nullptr, nullptr, nullptr, b, tiles, amp2, s2,
                     mean_c, acq, coef, best_value, tr_radius);
}

extern "C" void launch_psl_finalize_meanstd(
    const float* mu_part, const float* dist_part, const float* zq2,
    const float* quad, float* mean_out, float* sd_out, float* dist_out,
    int b, int tiles, float amp2, float s2, float mean_c,
    hipStream_t stream) {
  const int block = 256;
  hipLaunchKernelGGL(psl_finalize_kernel, dim3((b + block - 1) / block),
                     dim3(block), 0, stream, mu_part, dist_part, zq2, quad,
                     nullptr, mean_out, sd_out, dist_out, b, tiles, amp2, s2,
                     mean_c, 0, 0.0f, 0.0f, 0.0f);
}
