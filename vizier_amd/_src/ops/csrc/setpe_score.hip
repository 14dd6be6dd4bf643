// Set-PE logdet score over candidate SETS for gfx950 (fp32, wave64).
//
// Numeric spec: the set scorer of VizierGPUCBPEBandit (gp_ucb_pe.py,
// _set_pe_score_fn; reference SetPEScoreFunction / _logdet /
// _apply_trust_region_to_set). For each set b of q <= 16 candidates (rows
// b*q .. b*q+q-1 of the flattened batch):
//   A        = cov[b] + jitter I
//   logdet   = sum_j log(pivot_j) of the Cholesky of A, or -inf when a
//              pivot is not > 0 (NaN included): cholesky_ex's info > 0
//   penalty  = penalty_coef sum_m min(mean_m + explore_coef sd_m - thr, 0)
//   tr       = sum_m [dist_m > tr_radius] (-1e4 - dist_m)
//              (only with dist and 0 < tr_radius <= 0.5)
//   score[b] = logdet + penalty + tr
//
// The host builds cov and dist with the qEI stages A-C (ps_kvec_kernel, one
// K^-1 SGEMM, qei_cov_kernel) under the completed + pending posterior, and
// (mean, sd) with the posterior_mean_std sequence under the completed one;
// this kernel is the tail. Nothing uses atomics: every sum has a fixed
// order, so scores are bit-identical run to run and a captured sweep can be
// bit-compared with the eager one.

#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"

#define SETPE_QMAX 16
#define SETPE_WAVES 4  // sets per workgroup

// One wave per set, SETPE_WAVES sets per workgroup; the waves share
// nothing (no LDS, no barrier), so a bad set cannot touch its neighbours.
// The factorisation is the register-resident right-looking Cholesky of
// qei_mc_kernel: lane i owns row i, column j of the panel travels by wave
// shuffle, and every register index is a compile-time constant (full
// unroll to SETPE_QMAX, steps j >= q skipped by a wave-uniform branch).
// The pivot is the same in every lane, so each lane keeps the whole
// sum_j log(pivot_j) in step order.
extern "C" __global__ __launch_bounds__(SETPE_WAVES * WAVE_SIZE) void
setpe_logdet_kernel(const float* __restrict__ cov,   // (B, q, q)
                    const float* __restrict__ mean,  // (B*q,)
                    const float* __restrict__ sd,    // (B*q,)
                    const float* __restrict__ dist,  // (B*q,) or NULL
                    float* __restrict__ out,         // (B,)
                    int nb, int q, float jitter, float threshold,
                    float explore_coef, float penalty_coef,
                    float tr_radius) {
  const int b = blockIdx.x * SETPE_WAVES + threadIdx.x / WAVE_SIZE;
  if (b >= nb) return;  // wave-uniform
  const int i = threadIdx.x % WAVE_SIZE;  // row owned by this lane

  float a[SETPE_QMAX];
#pragma unroll
  for (int c = 0; c < SETPE_QMAX; ++c) {
    a[c] = (i < q && c < q) ? cov[((long)b * q + i) * q + c] : 0.0f;
    if (c == i) a[c] += jitter;
  }
  bool bad = false;
  float logdet = 0.0f;
#pragma unroll
  for (int j = 0; j < SETPE_QMAX; ++j) {
    if (j < q) {
      const float pivot = __shfl(a[j], j, WAVE_SIZE);
      // Not > 0 (NaN included): cholesky_ex's info > 0.
      if (!(pivot > 0.0f)) bad = true;
      logdet += logf(pivot);
      const float ljj = sqrtf(pivot);
      if (i == j) a[j] = ljj;
      if (i > j) a[j] = a[j] / ljj;
      // Trailing update A[i][c] -= L[i][j] L[c][j], j < c <= i.
#pragma unroll
      for (int c = j + 1; c < SETPE_QMAX; ++c) {
        if (c < q) {
          const float lcj = __shfl(a[j], c, WAVE_SIZE);
          if (c <= i) a[c] = fmaf(-a[j], lcj, a[c]);
        }
      }
    }
  }

  // Lane m holds member m; lanes >= q add exact zeros to the shuffle tree.
  float pen = 0.0f;
  float tr = 0.0f;
  if (i < q) {
    const long m = (long)b * q + i;
    const float v = fmaf(explore_coef, sd[m], mean[m]) - threshold;
    pen = v >= 0.0f ? 0.0f : v;  // the ?: keeps a NaN, as torch.minimum
    if (dist != nullptr && tr_radius > 0.0f && tr_radius <= 0.5f) {
      const float dd = dist[m];
      if (dd > tr_radius) tr = -1e4f - dd;
    }
  }
  pen = wave_reduce_sum(pen);
  tr = wave_reduce_sum(tr);
  if (i == 0) {
    out[b] = (bad ? -INFINITY : logdet) + penalty_coef * pen + tr;
  }
}

extern "C" void launch_setpe_logdet(
    const float* cov, const float* mean, const float* sd, const float* dist,
    float* out, int b, int q, float jitter, float threshold,
    float explore_coef, float penalty_coef, float tr_radius,
    hipStream_t stream) {
  const dim3 grid((b + SETPE_WAVES - 1) / SETPE_WAVES);
  const dim3 block(SETPE_WAVES * WAVE_SIZE);
  hipLaunchKernelGGL(setpe_logdet_kernel, grid, block, 0, stream, cov, mean,
                     sd, dist, out, b, q, jitter, threshold, explore_coef,
                     penalty_coef, tr_radius);
}
