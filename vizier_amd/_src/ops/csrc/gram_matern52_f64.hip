// fp64 Matern-5/2 ARD Gram / cross-Gram kernel for gfx950.
//
// K[i,j] = amp^2 * m52(||(x1_i - x2_j) * inv_ls||) for x1 (N,D), x2 (M,D)
// in double. Deliberately NOT a matrix-core kernel: D is small, and the
// difference form (never n1 + n2 - 2 x1.x2) is what makes the diagonal of
// a symmetric call exactly amp^2 (d2 = 0 -> sqrt(0) = 0 -> exp(-0) = 1).
// Same 16x16 LDS-tiled shape as the fp32 kernel in gram_matern52.hip.
//
// Numeric spec: vizier_amd/_src/gp/matern.py::gram_matern52 in float64.

#include <hip/hip_runtime.h>
#include "common.h"

#define TILE 16
#define DCHUNK 32

extern "C" __global__ __launch_bounds__(TILE * TILE) void
gram_matern52_f64_kernel(const double* __restrict__ x1,
                         const double* __restrict__ x2,
                         const double* __restrict__ inv_ls,  // (D,)
                         double* __restrict__ out, int n, int m, int d,
                         double amp2, int sym /* x1 == x2 */) {
  __shared__ double lds1[TILE][DCHUNK + 1];
  __shared__ double lds2[TILE][DCHUNK + 1];
  __shared__ double ldsl[DCHUNK];

  const int ty = threadIdx.x / TILE;   // row within tile
  const int tx = threadIdx.x % TILE;   // col within tile
  const int row0 = blockIdx.y * TILE;
  const int col0 = blockIdx.x * TILE;
  // Symmetric call: strictly-lower tiles are written by their mirror.
  if (sym && col0 + TILE <= row0) return;

  double acc = 0.0;
  for (int d0 = 0; d0 < d; d0 += DCHUNK) {
    const int dc = min(DCHUNK, d - d0);
    for (int c = tx; c < dc; c += TILE) {
      const int r1 = row0 + ty;
      const int r2 = col0 + ty;
      lds1[ty][c] = (r1 < n) ? x1[(long)r1 * d + d0 + c] : 0.0;
      lds2[ty][c] = (r2 < m) ? x2[(long)r2 * d + d0 + c] : 0.0;
    }
    if (ty == 0) {
      for (int c = tx; c < dc; c += TILE) ldsl[c] = inv_ls[d0 + c];
    }
    __syncthreads();
#pragma unroll 4
    for (int c = 0; c < dc; ++c) {
      const double z = (lds1[ty][c] - lds2[tx][c]) * ldsl[c];
      acc = fma(z, z, acc);
    }
    __syncthreads();
  }

  const int row = row0 + ty;
  const int col = col0 + tx;
  if (row < n && col < m) {
    const double k = amp2 * matern52_of_d2(acc);
    out[(long)row * m + col] = k;
    // Mirror the strictly-upper tiles; in the diagonal tile both (r, c)
    // and (c, r) are computed (bitwise equal: the difference only flips
    // sign before it is squared).
    if (sym && col0 > row0) out[(long)col * m + row] = k;
  }
}

extern "C" void launch_gram_matern52_f64(
    const double* x1, const double* x2, const double* inv_ls, double* out,
    int n, int m, int d, double amp2, int sym, hipStream_t stream) {
  dim3 grid((m + TILE - 1) / TILE, (n + TILE - 1) / TILE);
  hipLaunchKernelGGL(gram_matern52_f64_kernel, grid, dim3(TILE * TILE), 0,
                     stream, x1, x2, inv_ls, out, n, m, d, amp2, sym);
}
