// fp64 fused GP-posterior scorer for gfx950 (the float64 parity mode).
//
// Same three-step shape as the fp32 chunked scorer (posterior_score.hip),
// with `double` operands and ONE kernel sequence for every (B, N):
//
//   ps_kvec_f64       k[q,n] = amp^2 m52(||(xq_q - x_n) * inv_ls||),
//                     mu[q] = k_q . alpha, dist[q] = masked min-Linf
//   ps_quadform_f64   partials of quad[q] = k_q^T Kinv k_q on the fp64
//                     matrix cores (v_mfma_f64_16x16x4_f64)
//   ps_finalize_f64   fixed-order sum of the partials, variance clamp,
//                     acquisition, trust-region penalty
//
// No atomics anywhere: every partial has exactly one writer and the
// finalize kernel adds them in an order that depends only on (N, B), so
// two calls on the same operands return bitwise-equal results.
//
// Quadform tile mapping. One wave (64 lanes) owns a 16-column stripe of
// Kinv (columns j0..j0+15) and one slab of the reduction range over i.
// Per MFMA step T(16 candidates x 16 columns) += A(16x4) * B(4x16):
//   A[row][kk] = k[q0 + row][i + kk]      lane: row = lane & 15, kk = lane >> 4
//   B[kk][col] = Kinv[i + kk][j0 + col]   lane: col = lane & 15, kk = lane >> 4
//   T: 4 doubles per lane, col = lane & 15, row = (lane >> 4) + 4 * reg
// Out-of-range lanes (candidate >= B, i past the slab / N, column >= N)
// hold 0.0 and never form an address. The wave keeps two accumulator
// tiles (32 candidates) per pass over its slab, so for B <= 32 Kinv is
// read once per scorer call; B > 32 loops over further pairs of tiles.
// Epilogue: T[q][j] * k[q][j0 + j], summed over the 16 columns with a
// fixed xor-shuffle tree, one partial per (q, column tile, slab).

#include <hip/hip_runtime.h>
#include "common.h"

#define BLOCK 256

typedef double v4f64 __attribute__((ext_vector_type(4)));

// -- k-vector ----------------------------------------------------------------

extern "C" __global__ __launch_bounds__(BLOCK) void
ps_kvec_f64_kernel(const double* __restrict__ xq,      // (B, D)
                   const double* __restrict__ x,       // (N, D)
                   const double* __restrict__ inv_ls,  // (D,)
                   const double* __restrict__ alpha,   // (N,)
                   const unsigned char* __restrict__ onehot,  // (D,)
                   double* __restrict__ k_out,         // (B, N)
                   double* __restrict__ mu_out,        // (B,) without mean_c
                   double* __restrict__ dist_out,      // (B,)
                   int b, int n, int d, double amp2) {
  __shared__ double red[8];
  __shared__ double xq_lds[512];
  const int q = blockIdx.x;
  if (q >= b) return;
  const int tid = threadIdx.x;
  for (int j = tid; j < d; j += BLOCK) xq_lds[j] = xq[(long)q * d + j];
  __syncthreads();
  double mu_acc = 0.0;
  double min_linf = INFINITY;
  for (int row = tid; row < n; row += BLOCK) {
    const double* xr = x + (long)row * d;
    double d2 = 0.0, linf = 0.0;
    for (int j = 0; j < d; ++j) {
      const double diff = xq_lds[j] - xr[j];
      const double z = diff * inv_ls[j];
      d2 = fma(z, z, d2);
      if (!onehot[j]) linf = fmax(linf, fabs(diff));
    }
    const double kv = amp2 * matern52_of_d2(d2);
    k_out[(long)q * n + row] = kv;
    mu_acc = fma(kv, alpha[row], mu_acc);
    min_linf = fmin(min_linf, linf);
  }
  auto dsum = [](double a, double c) { return a + c; };
  auto dmin = [](double a, double c) { return fmin(a, c); };
  const double mu = block_reduce(mu_acc, red, dsum, 0.0);
  if (tid == 0) mu_out[q] = mu;
  __syncthreads();
  const double dist = block_reduce(min_linf, red, dmin, (double)INFINITY);
  if (tid == 0) dist_out[q] = dist;
}

// -- quadform on the fp64 matrix cores ----------------------------------------

// MFMA steps (4 rows of Kinv each) whose operand loads are issued together.
#define QF64_STEPS 4
// Waves the (column tile x slab) grid aims for: 256 CUs x 4 SIMDs x 2.
#define QF64_TARGET_WAVES 2048

// Slab decomposition of the reduction range, a function of n alone so the
// binding can size the workspace and the summation order is reproducible.
extern "C" void ps_f64_quadform_shape(int n, int* ctiles, int* slabs,
                                      int* slab_rows) {
  const int ct = (n + 15) / 16;
  int s = (QF64_TARGET_WAVES + ct - 1) / ct;
  if (s > ct) s = ct;  // at least 16 rows per slab
  if (s < 1) s = 1;
  int rows = ((n + s - 1) / s + 15) / 16 * 16;
  if (rows < 16) rows = 16;
  *ctiles = ct;
  *slab_rows = rows;
  *slabs = (n + rows - 1) / rows;
}

__device__ __forceinline__ double qf64_reduce16(double v) {
  // Sum over the 16 lanes that share lane >> 4 (the tile's columns).
#pragma unroll
  for (int m = 8; m > 0; m >>= 1) v += __shfl_xor(v, m, WAVE_SIZE);
  return v;
}

extern "C" __global__ __launch_bounds__(WAVE_SIZE) void
ps_quadform_f64_kernel(const double* __restrict__ k_in,   // (B, N)
                       const double* __restrict__ kinv,   // (N, N)
                       double* __restrict__ part,  // (B, ctiles * slabs)
                       int b, int n, int slab_rows, int slabs) {
  const int lane = threadIdx.x;
  const int lo = lane & 15, hi = lane >> 4;
  const int ct = blockIdx.x, slab = blockIdx.y;
  const long pstride = (long)gridDim.x * slabs;
  const int j = ct * 16 + lo;
  const bool jok = j < n;
  const int ibeg = slab * slab_rows;
  const int iend = min(n, ibeg + slab_rows);
  const int qtiles = (b + 15) / 16;
  for (int qt = 0; qt < qtiles; qt += 2) {
    const bool two = qt + 1 < qtiles;  // wave-uniform
    const int qa0 = qt * 16 + lo, qa1 = qa0 + 16;
    const bool q0ok = qa0 < b, q1ok = two && qa1 < b;
    v4f64 acc0 = {0.0, 0.0, 0.0, 0.0};
    v4f64 acc1 = {0.0, 0.0, 0.0, 0.0};
    for (int i0 = ibeg; i0 < iend; i0 += 4 * QF64_STEPS) {
      double bv[QF64_STEPS], a0[QF64_STEPS], a1[QF64_STEPS];
#pragma unroll
      for (int s = 0; s < QF64_STEPS; ++s) {
        const int i = i0 + 4 * s + hi;
        const bool iok = i < iend;
        bv[s] = (iok && jok) ? kinv[(long)i * n + j] : 0.0;
        a0[s] = (iok && q0ok) ? k_in[(long)qa0 * n + i] : 0.0;
        a1[s] = (iok && q1ok) ? k_in[(long)qa1 * n + i] : 0.0;
      }
#pragma unroll
      for (int s = 0; s < QF64_STEPS; ++s) {
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[s], bv[s], acc0,
                                                    0, 0, 0);
        if (two) {
          acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[s], bv[s], acc1,
                                                      0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q0 = qt * 16 + hi + 4 * r;
      const double kq0 = (q0 < b && jok) ? k_in[(long)q0 * n + j] : 0.0;
      const double v0 = qf64_reduce16(acc0[r] * kq0);
      if (lo == 0 && q0 < b) {
        part[(long)q0 * pstride + (long)ct * slabs + slab] = v0;
      }
      if (two) {
        const int q1 = q0 + 16;
        const double kq1 = (q1 < b && jok) ? k_in[(long)q1 * n + j] : 0.0;
        const double v1 = qf64_reduce16(acc1[r] * kq1);
        if (lo == 0 && q1 < b) {
          part[(long)q1 * pstride + (long)ct * slabs + slab] = v1;
        }
      }
    }
  }
}

// -- finalize ------------------------------------------------------------------

// One workgroup per candidate. Thread t adds partials t, t + 256, ... in
// index order, then the fixed block tree combines the 256 sums. Writes
// the score (out != nullptr) and/or mean and sd.
extern "C" __global__ __launch_bounds__(BLOCK) void
ps_finalize_f64_kernel(const double* __restrict__ mu_in,
                       const double* __restrict__ dist_in,
                       const double* __restrict__ part, long nparts,
                       double* __restrict__ out,
                       double* __restrict__ mean_out,
                       double* __restrict__ sd_out, int b, double amp2,
                       double mean_c, int acq, double coef,
                       double best_value, double tr_radius) {
  __shared__ double red[8];
  const int q = blockIdx.x;
  if (q >= b) return;
  const int tid = threadIdx.x;
  const double* p = part + (long)q * nparts;
  double acc = 0.0;
  for (long t = tid; t < nparts; t += BLOCK) acc += p[t];
  auto dsum = [](double a, double c) { return a + c; };
  const double quad = block_reduce(acc, red, dsum, 0.0);
  if (tid != 0) return;
  const double var = fmax(amp2 - quad, 1e-12);
  const double sd = sqrt(var);
  const double mu = mu_in[q] + mean_c;
  if (mean_out != nullptr) mean_out[q] = mu;
  if (sd_out != nullptr) sd_out[q] = sd;
  if (out == nullptr) return;
  const double score = vz_acq_score(acq, mu, sd, coef, best_value);
  out[q] = vz_trust_region(score, dist_in[q], tr_radius);
}

// -- launcher --------------------------------------------------------------------

// part must hold b * ctiles * slabs doubles (ps_f64_quadform_shape). out
// or (mean_out, sd_out) may be null.
extern "C" void launch_posterior_score_f64(
    const double* xq, const double* x, const double* inv_ls,
    const double* alpha, const double* kinv, const unsigned char* onehot,
    double* k_ws, double* mu_ws, double* dist_ws, double* part,
    double* out, double* mean_out, double* sd_out, int b, int n, int d,
    double amp2, double mean_c, int acq, double coef, double best_value,
    double tr_radius, hipStream_t stream) {
  int ctiles, slabs, slab_rows;
  ps_f64_quadform_shape(n, &ctiles, &slabs, &slab_rows);
  hipLaunchKernelGGL(ps_kvec_f64_kernel, dim3(b), dim3(BLOCK), 0, stream,
                     xq, x, inv_ls, alpha, onehot, k_ws, mu_ws, dist_ws, b,
                     n, d, amp2);
  hipLaunchKernelGGL(ps_quadform_f64_kernel, dim3(ctiles, slabs),
                     dim3(WAVE_SIZE), 0, stream, k_ws, kinv, part, b, n,
                     slab_rows, slabs);
  hipLaunchKernelGGL(ps_finalize_f64_kernel, dim3(b), dim3(BLOCK), 0,
                     stream, mu_ws, dist_ws, part, (long)ctiles * slabs,
                     out, mean_out, sd_out, b, amp2, mean_c, acq, coef,
                     best_value, tr_radius);
}
