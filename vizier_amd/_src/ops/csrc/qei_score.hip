// Monte-Carlo qEI over candidate SETS for gfx950 (fp32, wave64).
//
// Numeric spec: posterior_batched_cov (plain GPPosterior with K_inv) +
// acquisitions.qei_mc_scores + TrustRegion.apply(dense[:, 0, :], .).
// For each set b of q <= 16 candidates (rows b*q .. b*q+q-1 of the
// flattened batch):
//   mean[b][r]   = mean_c + k_r . alpha
//   cov[b][r][c] = amp^2 m52(||(x_r - x_c)/ls||) - k_r^T Kinv k_c
//   L            = chol(cov + 1e-4 max(mean(diag cov), 1e-10) I), or
//                  diag(sqrt(max(diag cov, 1e-12))) when a pivot is not > 0
//   score[b]     = mean_s max_r (mean_r + (L eps_s)_r - best)_+
//                  (or -1e4 - dist outside the trust region, by member 0)
//
// The host runs ps_kvec_kernel on the B*q flattened candidates (k-vectors,
// k . alpha, trust-region distance) and T = k @ Kinv as one SGEMM; the two
// kernels here do the q-specific rest. Nothing uses atomics: every sum has
// a fixed order, so scores are bit-identical run to run and a captured
// sweep can be bit-compared with the eager one.

#include <hip/hip_runtime.h>
#include "common.h"

#define QEI_COV_BLOCK 512
#define QEI_MC_BLOCK 128
#define QEI_QMAX 16

// -- Stage C: joint mean + covariance -------------------------------------
//
// One workgroup per set. Thread t walks n = t, t + BLOCK, ... and keeps the
// QMAX (QMAX + 1) / 2 lower-triangle partial sums of
//   Q[r][c] = sum_n T[b q + r][n] * k[b q + c][n]        (r >= c)
// in registers (2 q coalesced loads feed q (q + 1) / 2 fmas), then wave
// shuffle-reduces each and sums the wave partials in wave order. B is ~25
// sets, so the kernel is latency-bound: 512 threads keep the n walk at 4
// steps for N = 2000, and the candidates are staged in LDS so that the kqq
// pass after the barrier does not chain D global loads (13.3 us at config
// 3; 17.5 us with 256 threads and kqq from global memory, see
// profiles/bench_qei_hip.md). 512 threads is the most the ~190 VGPRs of
// the q = 16 instance allow.
//
// ASSUMES Kinv symmetric (gp_model builds it as z^T z): only r >= c is
// computed, T_r . k_c = k_r^T Kinv k_c, and the upper triangle is a mirror
// of the lower one. With a non-symmetric Kinv the upper triangle would be
// wrong; cov comes out exactly symmetric either way.
template <int QMAX>
__global__ __launch_bounds__(QEI_COV_BLOCK) void
qei_cov_kernel(const float* __restrict__ t_ws,    // (B*q, N) = k @ Kinv
               const float* __restrict__ k_ws,    // (B*q, N)
               const float* __restrict__ mu_ws,   // (B*q,) k . alpha
               const float* __restrict__ xs,      // (B, q, D)
               const float* __restrict__ inv_ls,  // (D,)
               float* __restrict__ mean_out,      // (B, q)
               float* __restrict__ cov_out,       // (B, q, q)
               int q, int n, int d, float amp2, float mean_c) {
  constexpr int NP = QMAX * (QMAX + 1) / 2;
  constexpr int WAVES = QEI_COV_BLOCK / WAVE_SIZE;
  __shared__ float part[NP][WAVES];
  __shared__ float xs_lds[QMAX * 512];  // the set's candidates (D <= 512)
  __shared__ float ils_lds[512];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  // Staged for the kqq pass below; the barrier after the reduction
  // publishes them.
  for (int e = tid; e < q * d; e += QEI_COV_BLOCK) {
    xs_lds[e] = xs[(long)b * q * d + e];
  }
  for (int j = tid; j < d; j += QEI_COV_BLOCK) ils_lds[j] = inv_ls[j];
  const float* tb = t_ws + (long)b * q * n;
  const float* kb = k_ws + (long)b * q * n;

  float acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = 0.0f;
  for (int i = tid; i < n; i += QEI_COV_BLOCK) {
    float tv[QMAX], kv[QMAX];
#pragma unroll
    for (int r = 0; r < QMAX; ++r) {
      // Rows r >= q belong to the next set (or lie past the workspace).
      tv[r] = r < q ? tb[(long)r * n + i] : 0.0f;
      kv[r] = r < q ? kb[(long)r * n + i] : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < QMAX; ++r) {
      if (r < q) {
#pragma unroll
        for (int c = 0; c <= r; ++c) {
          acc[r * (r + 1) / 2 + c] =
              fmaf(tv[r], kv[c], acc[r * (r + 1) / 2 + c]);
        }
      }
    }
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const float v = wave_reduce_sum(acc[p]);
    if (lane == 0) part[p][wave] = v;
  }
  __syncthreads();

  if (tid < q) mean_out[(long)b * q + tid] = mu_ws[(long)b * q + tid] + mean_c;

  // Thread p owns pair (r, c), p = r (r + 1) / 2 + c.
  if (tid < q * (q + 1) / 2) {
    int r = 0;
    while ((r + 1) * (r + 2) / 2 <= tid) ++r;
    const int c = tid - r * (r + 1) / 2;
    float quad = part[tid][0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) quad += part[tid][w];
    float kqq = amp2;  // the diagonal is exactly amp^2
    if (r != c) {
      const float* xr = xs_lds + r * d;
      const float* xc = xs_lds + c * d;
      float d2 = 0.0f;
      for (int j = 0; j < d; ++j) {
        const float z = (xr[j] - xc[j]) * ils_lds[j];
        d2 = fmaf(z, z, d2);
      }
      kqq = amp2 * matern52_of_d2(d2);
    }
    const float v = kqq - quad;
    float* cb = cov_out + (long)b * q * q;
    cb[r * q + c] = v;
    cb[c * q + r] = v;
  }
}

extern "C" void launch_qei_cov(
    const float* t_ws, const float* k_ws, const float* mu_ws,
    const float* xs, const float* inv_ls, float* mean_out, float* cov_out,
    int b, int q, int n, int d, float amp2, float mean_c,
    hipStream_t stream) {
  const dim3 grid(b), block(QEI_COV_BLOCK);
  if (q <= 4) {
    hipLaunchKernelGGL(qei_cov_kernel<4>, grid, block, 0, stream, t_ws,
                       k_ws, mu_ws, xs, inv_ls, mean_out, cov_out, q, n, d,
                       amp2, mean_c);
  } else if (q <= 8) {
    hipLaunchKernelGGL(qei_cov_kernel<8>, grid, block, 0, stream, t_ws,
                       k_ws, mu_ws, xs, inv_ls, mean_out, cov_out, q, n, d,
                       amp2, mean_c);
  } else {
    hipLaunchKernelGGL(qei_cov_kernel<QEI_QMAX>, grid, block, 0, stream,
                       t_ws, k_ws, mu_ws, xs, inv_ls, mean_out, cov_out, q,
                       n, d, amp2, mean_c);
  }
}

// -- Stage D: tiny Cholesky + Monte-Carlo max-improvement ------------------
//
// One workgroup per set. Wave 0 factors the jittered q x q covariance with
// a right-looking Cholesky held in REGISTERS: lane i owns row i, column j
// of the panel travels by wave shuffle, and every register index is a
// compile-time constant (full unroll to QEI_QMAX, steps j >= q skipped by a
// wave-uniform branch). L then goes to LDS (<= 1 KB), and all threads draw
// samples s = tid, tid + BLOCK, ...
extern "C" __global__ __launch_bounds__(QEI_MC_BLOCK) void
qei_mc_kernel(const float* __restrict__ mean,   // (B, q)
              const float* __restrict__ cov,    // (B, q, q)
              const float* __restrict__ eps,    // (S, q)
              const float* __restrict__ dist,   // (B*q,) or NULL
              float* __restrict__ out,          // (B,)
              int q, int s, float best_value, float tr_radius) {
  __shared__ float l_lds[QEI_QMAX][QEI_QMAX + 1];
  __shared__ float mean_lds[QEI_QMAX];
  __shared__ float red[8];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;

  if (tid < WAVE_SIZE) {
    const int i = tid;  // row owned by this lane
    float a[QEI_QMAX];
    // diag is the UN-jittered diagonal: the fallback uses it.
    float diag = 0.0f;
#pragma unroll
    for (int c = 0; c < QEI_QMAX; ++c) {
      a[c] = (i < q && c < q) ? cov[((long)b * q + i) * q + c] : 0.0f;
      if (c == i) diag = a[c];
    }
    float dsum = wave_reduce_sum(i < q ? diag : 0.0f);
    dsum = __shfl(dsum, 0, WAVE_SIZE);
    const float jitter = 1e-4f * fmaxf(dsum / (float)q, 1e-10f);
#pragma unroll
    for (int c = 0; c < QEI_QMAX; ++c) {
      if (c == i) a[c] += jitter;
    }
    bool bad = false;
#pragma unroll
    for (int j = 0; j < QEI_QMAX; ++j) {
      if (j < q) {
        const float pivot = __shfl(a[j], j, WAVE_SIZE);
        // Not > 0 (NaN included): cholesky_ex's info > 0.
        if (!(pivot > 0.0f)) bad = true;
        const float ljj = sqrtf(pivot);
        if (i == j) a[j] = ljj;
        if (i > j) a[j] = a[j] / ljj;
        // Trailing update A[i][c] -= L[i][j] L[c][j], j < c <= i.
#pragma unroll
        for (int c = j + 1; c < QEI_QMAX; ++c) {
          if (c < q) {
            const float lcj = __shfl(a[j], c, WAVE_SIZE);
            if (c <= i) a[c] = fmaf(-a[j], lcj, a[c]);
          }
        }
      }
    }
    // Fallback: independent marginals from the un-jittered diagonal. The
    // ?: keeps a NaN diagonal a NaN, as clamp_min does.
    const float sd = sqrtf(diag < 1e-12f ? 1e-12f : diag);
    if (i < q) {
#pragma unroll
      for (int c = 0; c < QEI_QMAX; ++c) {
        if (c < q) {
          float v = c <= i ? a[c] : 0.0f;
          if (bad) v = (c == i) ? sd : 0.0f;
          l_lds[i][c] = v;
        }
      }
      mean_lds[i] = mean[(long)b * q + i];
    }
  }
  __syncthreads();

  float acc = 0.0f;
  for (int si = tid; si < s; si += QEI_MC_BLOCK) {
    float e[QEI_QMAX];
#pragma unroll
    for (int c = 0; c < QEI_QMAX; ++c) {
      e[c] = c < q ? eps[(long)si * q + c] : 0.0f;
    }
    float imp = 0.0f;
#pragma unroll
    for (int r = 0; r < QEI_QMAX; ++r) {
      if (r < q) {
        // y = L eps (NOT L^T eps): covariance L L^T = cov.
        float y = mean_lds[r];
#pragma unroll
        for (int c = 0; c <= r; ++c) y = fmaf(l_lds[r][c], e[c], y);
        imp = fmaxf(imp, y - best_value);
      }
    }
    acc += imp;
  }
  auto fsum = [](float x, float y) { return x + y; };
  const float total = block_reduce(acc, red, fsum, 0.0f);
  if (tid == 0) {
    float score = total / (float)s;
    if (dist != nullptr) {
      // Member 0 of the set decides, as TrustRegion.apply(dense[:, 0, :]).
      const float dd = dist[(long)b * q];
      if (tr_radius > 0.0f && tr_radius <= 0.5f && dd > tr_radius) {
        score = -1e4f - dd;
      }
    }
    out[b] = score;
  }
}

extern "C" void launch_qei_mc(
    const float* mean, const float* cov, const float* eps,
    const float* dist, float* out, int b, int q, int s, float best_value,
    float tr_radius, hipStream_t stream) {
  hipLaunchKernelGGL(qei_mc_kernel, dim3(b), dim3(QEI_MC_BLOCK), 0, stream,
                     mean, cov, eps, dist, out, q, s, best_value,
                     tr_radius);
}
