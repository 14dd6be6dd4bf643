// Double-precision helpers for the fp64 (parity mode) gfx950 kernels.
//
// The fp32 helpers in common.h stay untouched; everything here is the
// `double` counterpart. The RNG draws the SAME integers as the fp32
// kernels for the same (seed, offset, idx) (vz_splitmix64 from common.h)
// and widens them: the 24-bit uniform is exact in both formats, Laplace
// and Gumbel are evaluated in double from it.
#pragma once

#include <hip/hip_runtime.h>
#include "common.h"

__device__ __forceinline__ double vz_matern52_of_d2_f64(double d2) {
  // k(r) = (1 + sqrt5*r + 5r^2/3) exp(-sqrt5*r), r = sqrt(d2). sqrt and
  // exp are the correctly-rounded / <1 ulp double routines, not the fast
  // fp32 intrinsics.
  const double sr = 2.23606797749978969641 * sqrt(fmax(d2, 0.0));
  return (1.0 + sr + sr * sr / 3.0) * exp(-sr);
}

// Block-level reduction of doubles: up to 4 waves -> LDS -> wave 0. The
// shuffle tree and the LDS pass have a fixed shape, so the result is
// run-to-run deterministic. Valid in wave 0 lane 0.
template <typename Op>
__device__ __forceinline__ double block_reduce_f64(double v, double* lds4,
                                                   Op op, double init) {
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
#pragma unroll
  for (int offset = WAVE_SIZE / 2; offset > 0; offset >>= 1) {
    v = op(v, __shfl_down(v, offset, WAVE_SIZE));
  }
  if (lane == 0) lds4[wave] = v;
  __syncthreads();
  if (wave == 0) {
    v = (lane < blockDim.x / WAVE_SIZE) ? lds4[lane] : init;
#pragma unroll
    for (int offset = 2; offset > 0; offset >>= 1) {
      v = op(v, __shfl_down(v, offset, WAVE_SIZE));
    }
  }
  return v;
}

// Same 24-bit value as vz_rng_uniform: ((h >> 40) + 0.5) / 2^24, exact in
// double (25 significant bits).
__device__ __forceinline__ double vz_rng_uniform_f64(
    unsigned long long seed, unsigned long long offset, unsigned int idx) {
  const unsigned long long h =
      vz_splitmix64(seed ^ vz_splitmix64(offset ^ idx));
  return ((double)(h >> 40) + 0.5) * (1.0 / 16777216.0);
}

__device__ __forceinline__ double vz_rng_laplace_f64(
    unsigned long long seed, unsigned long long offset, unsigned int idx) {
  const double u = vz_rng_uniform_f64(seed, offset, idx) - 0.5;
  const double a = fmin(fabs(u), 0.499999);
  return (u >= 0.0 ? -1.0 : 1.0) * log1p(-2.0 * a);
}

__device__ __forceinline__ double vz_normal_cdf_f64(double z) {
  return 0.5 * erfc(-z * 0.70710678118654752440);
}
__device__ __forceinline__ double vz_normal_pdf_f64(double z) {
  return 0.39894228040143267794 * exp(-0.5 * z * z);
}
