// Batched Cholesky + forward substitution for the NLL line search
// (gfx950). MAGMA's batched spotf2 panels cost ~54 ms per suggest at
// the headline shape (16 x 1000 x 1000 per L-BFGS iteration,
// profiles/sweep_kernels_r2.txt) in ~5000 tiny kernel launches, and
// the (R, N, 1) triangular solves dispatch as SERIAL rocblas trsv
// calls (~170 us each). This file holds a right-looking blocked
// factorization in rounds of NB = 32 columns, two launches per round
// (panel, then trailing update) with the work of each spread over an
// (R x tiles) grid, and a blocked forward substitution that runs one
// workgroup per matrix. Forward-only: the autograd value_and_grad path
// keeps torch's factorization; the line-search (torch.no_grad) calls
// these.
//
// Factorization, two implementations with bit-identical lower triangles
// (tests/test_potrf_tiled.py; launch_batched_potrf takes `impl`):
//   - v6 (default): one-wave panel workgroups of 64 rows with a
//     column-wise solve, trailing update on 64 x 64 tiles. 0.53 / 0.63 /
//     0.71 ms at N = 1000, R = 2 / 8 / 16 (profiles/bench_potrf_tiled.md);
//   - v2: 256-row panel workgroups with a row-wise solve, trailing update
//     on 64-column strips. 2.8 ms at N = 1000 whatever R. Kept as the bit
//     oracle that v6 is held to.
// v1, v3, v4 and v5 were measured, lost and were removed; DESIGN.md
// ("Batched Cholesky saga", "Batched-Cholesky negative results") has what
// they were and their numbers.
//
// Forward substitution, two kernels with bit-identical results
// (tests/test_trsv_variants.py; launch_batched_trsv_lower picks):
//   - batched_trsv_lower_pipe_kernel (default, N <= 1280): every row's
//     accumulator and its L columns stay in registers, the diagonal block
//     is fetched one panel ahead and the panel's columns load while the
//     32-step chain runs, one block barrier per panel;
//   - batched_trsv_lower_kernel (variant 1, and N > 1280): stages the
//     panel's columns through LDS and read-modify-writes rhs in global
//     memory, two barriers per 256-row chunk, nothing prefetched.
// Measured at 16 x 1000 x 1000 (profiles/bench_resident_trsv.md): 632 ->
// 146 us per call, the b.clone() of the binding included.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.h"

#define CB 256
#define NB 32

// Blocked forward substitution: solves L z = b in place for (R, N)
// right-hand sides. Wave 0 runs the wave-synchronous 32-panel solve
// (shfl broadcasts, no block syncs inside the panel); all waves apply
// the trailing update.
extern "C" __global__ __launch_bounds__(CB) void
batched_trsv_lower_kernel(const float* __restrict__ L,  // (R, N, N)
                          float* __restrict__ b,        // (R, N)
                          int r_count, int n) {
  __shared__ float zseg[NB];
  __shared__ float rows_lds[CB][NB + 1];
  const int r = blockIdx.x;
  if (r >= r_count) return;
  const float* M = L + (long)r * n * n;
  float* rhs = b + (long)r * n;
  const int tid = threadIdx.x;
  const int lane = tid % WAVE_SIZE;

  for (int k0 = 0; k0 < n; k0 += NB) {
    const int nb = min(NB, n - k0);
    if (tid < WAVE_SIZE) {
      // Lane l preloads ITS row of the 32x32 diagonal block into
      // registers up front (one parallel burst), so the serial
      // 32-step substitution touches only registers + shfl. The
      // previous form read M inside the chain — 32 dependent L2
      // round trips per panel, ~800 us per 1000-row solve
      // (profiles/fit_kernels_headline3.txt).
      float row[NB];
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        row[c] = (lane < nb && c < nb && c <= lane)
            ? M[(long)(k0 + lane) * n + k0 + c] : 0.0f;
      }
      float myv = (lane < nb) ? rhs[k0 + lane] : 0.0f;
      for (int j = 0; j < nb; ++j) {
        float zj = 0.0f;
        if (j == lane) {
          zj = myv / row[j];
          zseg[j] = zj;
        }
        zj = __shfl(zj, j, WAVE_SIZE);
        if (lane > j && lane < nb) {
          myv = fmaf(-row[j], zj, myv);
        }
      }
      if (lane < nb) rhs[k0 + lane] = zseg[lane];
    }
    __syncthreads();
    // Row blocks staged through LDS for coalesced L-column reads.
    for (int i0 = k0 + nb; i0 < n; i0 += CB) {
      const int blk = min(CB, n - i0);
      for (int e = tid; e < blk * nb; e += CB) {
        rows_lds[e / nb][e % nb] =
            M[(long)(i0 + e / nb) * n + k0 + e % nb];
      }
      __syncthreads();
      const int i = i0 + tid;
      if (i < n) {
        float acc = rhs[i];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          if (j < nb) acc = fmaf(-rows_lds[tid][j], zseg[j], acc);
        }
        rhs[i] = acc;
      }
      __syncthreads();
    }
  }
}

// -- Pipelined forward substitution (default) ----------------------------
//
// Same arithmetic as batched_trsv_lower_kernel, row by row:
//   acc = b[i]; acc = fmaf(-L[i][j], z[j], acc) for j = 0 .. i-1 in column
//   order; z[i] = acc / L[i][i]
// so z is bit-identical. What changes is where the operands wait:
//   - thread t owns rows t, t + 256, ... (RPT of them) and keeps their
//     accumulators in registers for the whole solve: no read-modify-write
//     of rhs in global memory;
//   - it reads L[i][k0 .. k0+31] (one 128-byte line) straight into
//     registers, as float4 when VEC (n % 4 == 0, 16-byte aligned base),
//     and only for rows below the panel: no LDS transpose, two block
//     barriers per panel become one;
//   - the 32 rows of diagonal block k are rows of 32 consecutive threads
//     (256 is a multiple of 32): half of wave (k % 8) / 2. That half-wave
//     already holds their accumulators, so it runs the 32-step chain in
//     place, broadcasting z[j] with v_readlane;
//   - the diagonal block of panel k + 1 is fetched one panel ahead, and
//     the other three waves' columns of panel k are in flight while the
//     chain of panel k runs, so the chain itself never waits on memory.
// What is left per panel (146 us / 32 at N = 1000) is the chain, of the
// order of 1.7 us of dependent divide / readlane / fma, the chain wave's
// own column loads, which land after it, and the address-per-lane loads
// themselves: one float4 per lane per line, 8 instructions per row.
// The strict upper triangle of a diagonal block is loaded with its row but
// only ever selected away: lane l divides by dg[l] and multiplies dg[j] for
// j < l.
#define TRSV_PIPE_MAX_RPT 5

template <bool VEC>
__device__ __forceinline__ void trsv_load_row(const float* __restrict__ p,
                                              int ncols, float out[NB]) {
  if (VEC) {
#pragma unroll
    for (int q = 0; q < NB / 4; ++q) {
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (4 * q < ncols) v = *reinterpret_cast<const float4*>(p + 4 * q);
      out[4 * q] = v.x;
      out[4 * q + 1] = v.y;
      out[4 * q + 2] = v.z;
      out[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int c = 0; c < NB; ++c) out[c] = (c < ncols) ? p[c] : 0.0f;
  }
}

template <int RPT, bool VEC>
__global__ __launch_bounds__(CB) void
batched_trsv_lower_pipe_kernel(const float* __restrict__ L,  // (R, N, N)
                               float* __restrict__ b,        // (R, N)
                               int r_count, int n) {
  __shared__ float zseg[2][NB];  // double-buffered: one barrier per panel
  const int r = blockIdx.x;
  if (r >= r_count) return;
  const float* M = L + (long)r * n * n;
  float* rhs = b + (long)r * n;
  const int tid = threadIdx.x;
  const int lane = tid % WAVE_SIZE;
  const int wave = tid / WAVE_SIZE;
  const int l = tid % NB;    // row of a diagonal block this thread owns
  const int blk = tid / NB;  // ... in the panels with k % 8 == blk

  float acc[RPT];
  float cur[RPT][NB];
#pragma unroll
  for (int s = 0; s < RPT; ++s) {
    const int i = tid + s * CB;
    acc[s] = (i < n) ? rhs[i] : 0.0f;
#pragma unroll
    for (int c = 0; c < NB; ++c) cur[s][c] = 0.0f;
  }
  float dg[NB], dgn[NB];
#pragma unroll
  for (int c = 0; c < NB; ++c) dg[c] = dgn[c] = 0.0f;
  if (blk == 0 && l < n) trsv_load_row<VEC>(M + (long)l * n, min(NB, n), dg);

  const int npanels = (n + NB - 1) / NB;
  for (int k = 0; k < npanels; ++k) {
    const int k0 = k * NB;
    const int nb = min(NB, n - k0);
    const int below = k0 + nb;  // < n only after a full panel

    // Columns of this panel for the rows below it, and the next diagonal
    // block: in flight while the chain runs.
    auto issue_loads = [&]() {
#pragma unroll
      for (int s = 0; s < RPT; ++s) {
        const int i = tid + s * CB;
        if (i >= below && i < n) {
          trsv_load_row<VEC>(M + (long)i * n + k0, NB, cur[s]);
        }
      }
      const int k1 = k0 + NB;
      if (blk == ((k + 1) & 7) && k1 + l < n) {
        trsv_load_row<VEC>(M + (long)(k1 + l) * n + k1, min(NB, n - k1),
                           dgn);
      }
    };
    // The wave that runs the chain issues its loads after it: 64 lanes
    // x 8 float4 per row each touch their own line, and queueing those
    // ahead of the chain delayed it by more than the loads' latency
    // costs afterwards (175 -> 146 us per call, 16 x 1000 x 1000).
    const bool owner = wave == ((k & 7) >> 1);
    if (!owner) issue_loads();

    if (owner) {
      const int h = (k & 1) * NB;  // first lane of the owning half-wave
      const int sd = k0 / CB;      // the owners' slot of these rows
      float myv = 0.0f;
#pragma unroll
      for (int s = 0; s < RPT; ++s) {
        if (s == sd) myv = acc[s];
      }
      const int ll = lane - h;     // == l in the owning half, else outside
      const bool mine = ll >= 0 && ll < nb;
      float myz = 0.0f;
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        if (j >= nb) break;
        float zj = 0.0f;
        if (ll == j) {
          zj = myv / dg[j];
          myz = zj;
        }
        zj = __int_as_float(
            __builtin_amdgcn_readlane(__float_as_int(zj), h + j));
        if (mine && ll > j) {
          myv = fmaf(-dg[j], zj, myv);
        }
      }
      if (mine) {
        zseg[k & 1][ll] = myz;
        rhs[k0 + ll] = myz;
      }
      issue_loads();
    }
    __syncthreads();

    if (below < n) {
      float zs[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) zs[j] = zseg[k & 1][j];
#pragma unroll
      for (int s = 0; s < RPT; ++s) {
        const int i = tid + s * CB;
        if (i >= below && i < n) {
          float a = acc[s];
#pragma unroll
          for (int j = 0; j < NB; ++j) a = fmaf(-cur[s][j], zs[j], a);
          acc[s] = a;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < NB; ++c) dg[c] = dgn[c];
  }
}

// -- v2: the bit oracle ---------------------------------------------------
//
// Two launches per 32-column round (63 for N = 1000). The panel kernel
// runs a (R x 256-row tiles) grid: every workgroup factors the 32 x 32
// diagonal block itself and solves its own rows of L21 = A21 L11^-T, one
// row per thread. The trailing kernel runs a (R x 64-column strips) grid:
// a strip's workgroup walks every row below it, one thread per row. Those
// two serial chains, not launches or fences, are v2's ~40-50 us per kernel
// (see the v6 header); v6 computes the same bits faster, and
// tests/test_potrf_tiled.py holds it to what these kernels produce.

// No workgroup reads a diagonal block that another workgroup of the same
// launch writes. With one row tile (gridDim.y == 1) the only workgroup
// of a matrix factors the block and writes it in place. With more, every
// workgroup reads the UNFACTORED block, so workgroup y == 0 must not
// overwrite it in this launch: a workgroup that starts late (R x rtiles
// beyond what the chip holds at once; dispatch order is not a contract)
// would factor the factored block and write a wrong L21 slice. When the
// block was written in place, 2048 copies of a positive definite N = 321
// matrix all came back with info = 289. It parks the factor in
// `dscratch` (R, NB, NB) instead, and workgroup (r, 0) of this round's
// trailing kernel, which never reads the diagonal block, copies it into
// place. `dscratch` is null when the launch has one row tile.

extern "C" __global__ __launch_bounds__(CB) void
batched_potrf_panel_kernel(float* __restrict__ A, int* __restrict__ info,
                           float* __restrict__ dscratch, int r_count,
                           int n, int k0) {
  __shared__ float diag[NB][NB + 1];
  __shared__ float rows_lds[CB][NB + 1];
  const int r = blockIdx.x;
  if (r >= r_count) return;
  // Grid (R, row-tiles): each workgroup REDUNDANTLY factors the 32x32
  // diagonal block (deterministic, cheap — wave-synchronous with shfl
  // broadcasts) then solves its OWN CB-row slice of the column panel
  // L21 = A21 L11^-T. The r2 single-workgroup-per-matrix version put
  // ~70 us x 32 panels on 3 CUs at the headline shape (R=3, N=1000,
  // profiles/fit_kernels_headline.txt); slicing rows across blockIdx.y
  // lets the panel use the chip, and the panel block is staged through
  // LDS so global accesses are COALESCED (one thread per row reads a
  // 128-byte segment strided n*4 from its neighbor's — measured ~52 us
  // per launch before staging, launch floor is ~4.5 us).
  const int row0 = k0 + NB + blockIdx.y * CB;
  const bool has_rows = row0 < n;
  if (blockIdx.y > 0 && !has_rows) return;
  float* M = A + (long)r * n * n;
  const int tid = threadIdx.x;
  const int nb = min(NB, n - k0);
  if (tid < WAVE_SIZE) {
    const int lane = tid;
    float row[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      row[c] = (lane < nb && c < nb)
          ? M[(long)(k0 + lane) * n + k0 + c] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if (j >= nb) break;
      const float piv = __shfl(row[j], j, WAVE_SIZE);
      float d;
      if (piv > 0.0f) {
        d = sqrtf(piv);
      } else {
        d = 1.0f;
        if (blockIdx.y == 0 && lane == 0 && info[r] == 0) {
          info[r] = k0 + j + 1;
        }
      }
      if (lane == j) row[j] = d;
      if (lane > j) row[j] /= d;
#pragma unroll
      for (int c = 0; c < NB; ++c) {
        if (c > j && c < nb) {
          const float lcj = __shfl(row[j], c, WAVE_SIZE);
          if (lane >= c) row[c] -= row[j] * lcj;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      if (lane < nb && c < nb) diag[lane][c] = row[c];
    }
  }
  __syncthreads();
  if (blockIdx.y == 0) {
    float* ds = dscratch ? dscratch + (long)r * NB * NB : nullptr;
    for (int e = tid; e < nb * nb; e += CB) {
      const int i = e / nb, c = e % nb;
      const float v = (c <= i) ? diag[i][c] : 0.0f;
      if (ds) {
        ds[e] = v;
      } else {
        M[(long)(k0 + i) * n + k0 + c] = v;
      }
    }
  }
  const int tile_rows = has_rows ? min(CB, n - row0) : 0;
  for (int e = tid; e < tile_rows * nb; e += CB) {
    rows_lds[e / nb][e % nb] = M[(long)(row0 + e / nb) * n + k0 + e % nb];
  }
  __syncthreads();
  if (tid < tile_rows) {  // one row per thread in this tile
    float v[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if (j < nb) {
        float xv = rows_lds[tid][j];
#pragma unroll
        for (int p = 0; p < NB; ++p) {
          if (p < j) xv -= v[p] * diag[j][p];
        }
        v[j] = xv / diag[j][j];
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if (j < nb) rows_lds[tid][j] = v[j];
    }
  }
  __syncthreads();
  for (int e = tid; e < tile_rows * nb; e += CB) {
    M[(long)(row0 + e / nb) * n + k0 + e % nb] = rows_lds[e / nb][e % nb];
  }
}

extern "C" __global__ __launch_bounds__(CB) void
batched_potrf_trailing_kernel(float* __restrict__ A,
                              const float* __restrict__ dscratch,
                              int r_count, int n, int k0) {
  __shared__ float jpanel[64][NB];
  __shared__ float rows_lds[CB][NB + 1];
  const int r = blockIdx.x;
  if (r >= r_count) return;
  float* M = A + (long)r * n * n;
  const int tid = threadIdx.x;
  const int nb = min(NB, n - k0);
  if (dscratch != nullptr && blockIdx.y == 0) {
    // The factored diagonal block the panel kernel parked. Nothing in
    // this launch reads rows k0 .. k0 + nb.
    const float* ds = dscratch + (long)r * NB * NB;
    for (int e = tid; e < nb * nb; e += CB) {
      M[(long)(k0 + e / nb) * n + k0 + e % nb] = ds[e];
    }
  }
  const int jb = k0 + nb + blockIdx.y * 64;
  if (jb >= n) return;
  const int jl = min(64, n - jb);
  for (int e = tid; e < jl * nb; e += CB) {
    jpanel[e / nb][e % nb] = M[(long)(jb + e / nb) * n + k0 + e % nb];
  }
  __syncthreads();
  // Row blocks staged through LDS for coalesced panel reads (the
  // per-thread row loads are 4-KB-strided otherwise).
  for (int i0 = jb; i0 < n; i0 += CB) {
    const int blk = min(CB, n - i0);
    for (int e = tid; e < blk * nb; e += CB) {
      rows_lds[e / nb][e % nb] =
          M[(long)(i0 + e / nb) * n + k0 + e % nb];
    }
    __syncthreads();
    const int i = i0 + tid;
    if (i < n) {
      float row[NB];
#pragma unroll
      for (int p = 0; p < NB; ++p) {
        row[p] = (p < nb) ? rows_lds[tid][p] : 0.0f;
      }
      for (int j = 0; j < jl; ++j) {
        if (jb + j > i) break;
        float acc = 0.0f;
#pragma unroll
        for (int p = 0; p < NB; ++p) {
          acc = fmaf(row[p], jpanel[j][p], acc);
        }
        M[(long)i * n + jb + j] -= acc;
      }
    }
    __syncthreads();
  }
}

// -- v6 (default): v2's rounds with the work split differently -----------
//
// Same two launches per round, same parking rule for the diagonal block
// and, element by element, the same floating-point operations in the same
// order as v2, so the lower triangle of L is bit-identical
// (tests/test_potrf_tiled.py). v2's ~40-50 us per kernel was the length of
// the dependent chain on its critical workgroup, not work and not a fence:
//   - trailing: v2's strip-0 workgroup walks all the rows below it, one
//     thread per row, with a 4-KB-strided read-modify-write of M. v6 runs
//     one workgroup per 64 x 64 tile of the lower triangle, 4 x 4 outputs
//     per thread from two p-major LDS slices;
//   - panel: v2's wave factor broadcasts through LDS permutes and its row
//     solve is a 528-fma dependent chain per row fed by scalar LDS reads.
//     v6 broadcasts with v_readlane and solves column by column: for p
//     ascending v[p] = x[p] / d[p][p], then x[j] -= v[p] d[j][p] for all
//     j > p at once. Every x[j] still sees p ascending, so the bits are
//     v2's; the chain is 32 x (divide + fma). Rows go global -> registers
//     -> global, issued before the factor, and a workgroup is one wave of
//     64 rows: no block barrier. 64 rows beat 256 (one factoring wave,
//     three waiting) by 4 to 6 % of a factorization at every shape timed
//     (profiles/bench_potrf_tiled.md).

#define PANEL_ROWS 64  // rows per v6 panel workgroup: one per lane
#define TT 64          // edge of a trailing tile
#define TLD (TT + 4)   // p-major LDS row: padded, still 16-byte aligned

// Row `row` of M, columns col0 .. col0 + 31, into registers. Indices are
// clamped into the matrix instead of predicated, so all the loads issue
// back to back and nothing waits in between; what a clamp duplicates is
// never used by the caller. VEC needs n % 4 == 0, col0 % 4 == 0 and a
// 16-byte aligned M.
template <bool VEC>
__device__ __forceinline__ void potrf_load_row(const float* __restrict__ M,
                                               int n, int row, int col0,
                                               float out[NB]) {
  const float* p = M + (long)min(row, n - 1) * n;
  if (VEC) {
#pragma unroll
    for (int q = 0; q < NB / 4; ++q) {
      const float4 v =
          *reinterpret_cast<const float4*>(p + min(col0 + 4 * q, n - 4));
      out[4 * q] = v.x;
      out[4 * q + 1] = v.y;
      out[4 * q + 2] = v.z;
      out[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int c = 0; c < NB; ++c) out[c] = p[min(col0 + c, n - 1)];
  }
}

template <bool VEC>
__device__ __forceinline__ void potrf_store_row(float* __restrict__ p,
                                                int ncols,
                                                const float v[NB]) {
  if (VEC) {
#pragma unroll
    for (int q = 0; q < NB / 4; ++q) {
      if (4 * q < ncols) {
        *reinterpret_cast<float4*>(p + 4 * q) =
            make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      if (c < ncols) p[c] = v[c];
    }
  }
}

__device__ __forceinline__ float potrf_readlane(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// v2's row solve `xv -= v[p] * diag[j][p]` is not one fma throughout. As
// hipcc compiles it, the vectorizer pairs the multiplies of the last
// min(10, j rounded down to even) steps of column j into packed multiplies,
// whose products are rounded before the subtraction; the earlier steps
// contract to fma (read off the optimized IR and the ISA: 130 v_pk_mul_f32
// and 260 v_sub_f32 next to 268 fused steps). L depends on that split, so
// v6 spells it out, and tests/test_potrf_tiled.py fails if a compiler
// splits v2 differently.
__host__ __device__ constexpr bool potrf_solve_rounds_product(int j, int p) {
  return p >= j - ((j & ~1) < 10 ? (j & ~1) : 10);
}

__device__ __forceinline__ float potrf_sub_rounded_product(float x, float a,
                                                           float b) {
#pragma clang fp contract(off)
  const float prod = a * b;
  return x - prod;
}

// Grid (R, row tiles of 64), one wave. As in v2 every workgroup
// factors the diagonal block itself and workgroup y == 0 writes it out: in
// place when it is the matrix's only workgroup, else parked in `dscratch`.
// A partial last block (nb < 32, no rows below it) is padded with the
// identity: the padding's pivots are 1 and its multipliers 0, so the
// nb x nb corner sees exactly the operations of a factor of width nb and
// the wave factor needs no `c < nb` predicates.
template <bool VEC>
__global__ __launch_bounds__(PANEL_ROWS) void
batched_potrf_panel_cols_kernel(float* __restrict__ A,
                                int* __restrict__ info,
                                float* __restrict__ dscratch, int n,
                                int k0) {
  // dcol[p][j] = d[j][p]: what column step p of the solve reads is
  // contiguous, and a b128 read of it is one broadcast.
  __shared__ __attribute__((aligned(16))) float dcol[NB][NB];
  const int r = blockIdx.x;
  float* M = A + (long)r * n * n;
  static_assert(PANEL_ROWS == WAVE_SIZE, "one wave factors and solves");
  const int lane = threadIdx.x;
  const int nb = min(NB, n - k0);
  const int i = k0 + NB + (int)blockIdx.y * PANEL_ROWS + lane;

  float x[NB], row[NB];
  potrf_load_row<VEC>(M, n, i, k0, x);
  potrf_load_row<VEC>(M, n, k0 + lane, k0, row);
#pragma unroll
  for (int c = 0; c < NB; ++c) {
    if (lane >= nb || c >= nb) row[c] = (c == lane) ? 1.0f : 0.0f;
  }
  // Lane l < 32 holds row l of the block. Entries above the diagonal
  // carry values nobody reads (v2 masks them off instead): only d[j][p]
  // with p <= j is ever used or stored.
  int fc = 0;
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const float piv = potrf_readlane(row[j], j);
    const bool ok = piv > 0.0f;
    const float d = ok ? sqrtf(piv) : 1.0f;
    if (!ok && fc == 0) fc = k0 + j + 1;
    row[j] = (lane == j) ? d : row[j] / d;
#pragma unroll
    for (int c = j + 1; c < NB; ++c) {
      const float lcj = potrf_readlane(row[j], c);
      row[c] = fmaf(-row[j], lcj, row[c]);
    }
  }
  if (lane < NB) {
#pragma unroll
    for (int c = 0; c < NB; ++c) dcol[c][lane] = row[c];
  }
  __syncthreads();
  if (blockIdx.y == 0 && lane < nb) {
#pragma unroll
    for (int c = 0; c < NB; ++c) {
      if (c > lane) row[c] = 0.0f;
    }
    float* dst = dscratch != nullptr
        ? dscratch + (long)r * NB * NB + lane * NB
        : M + (long)(k0 + lane) * n + k0;
    potrf_store_row<VEC>(dst, nb, row);
    if (lane == 0 && fc != 0 && info[r] == 0) info[r] = fc;
  }
  if (k0 + NB >= n) return;  // uniform: no rows below this block

  // Lanes past the last row solve a clamped copy and store nothing.
#pragma unroll
  for (int p = 0; p < NB; ++p) {
    float dc[NB];
#pragma unroll
    for (int q = p / 4; q < NB / 4; ++q) {
      const float4 v = *reinterpret_cast<const float4*>(&dcol[p][4 * q]);
      dc[4 * q] = v.x;
      dc[4 * q + 1] = v.y;
      dc[4 * q + 2] = v.z;
      dc[4 * q + 3] = v.w;
    }
    const float v = x[p] / dc[p];
    x[p] = v;
#pragma unroll
    for (int j = p + 1; j < NB; ++j) {
      x[j] = potrf_solve_rounds_product(j, p)
          ? potrf_sub_rounded_product(x[j], v, dc[j])
          : fmaf(-v, dc[j], x[j]);
    }
  }
  if (i < n) potrf_store_row<VEC>(M + (long)i * n + k0, NB, x);
}

// Grid (R x lower-triangular tile pairs ti >= tj of the trailing matrix),
// flattened so that R is not bound by gridDim.y; 256 threads, thread
// (ty, tx) owns the 4 x 4 outputs at rows ib + 4 ty, columns jb + 4 tx.
// Only full panels have a trailing matrix, so nb == 32 here. Per element
// acc = 0; acc = fmaf(L[i][k0 + p], L[j][k0 + p], acc), p ascending;
// M[i][j] -= acc, as in v2. The pair's first workgroup copies the parked
// diagonal block into place (rows k0 .. k0 + 31: read by nobody here).
template <bool VEC>
__global__ __launch_bounds__(CB) void
batched_potrf_trailing_tiled_kernel(float* __restrict__ A,
                                    const float* __restrict__ dscratch,
                                    int n, int k0, int pairs) {
  __shared__ __attribute__((aligned(16))) float As[NB][TLD];
  __shared__ __attribute__((aligned(16))) float Bs[NB][TLD];
  const int r = blockIdx.x / pairs;
  const int pair = blockIdx.x % pairs;
  float* M = A + (long)r * n * n;
  const int tid = threadIdx.x;

  if (dscratch != nullptr && pair == 0) {
    const float* ds = dscratch + (long)r * NB * NB;
    if (VEC) {
      const int di = tid / (NB / 4), dq = tid % (NB / 4);
      *reinterpret_cast<float4*>(M + (long)(k0 + di) * n + k0 + 4 * dq) =
          *reinterpret_cast<const float4*>(ds + di * NB + 4 * dq);
    } else {
      for (int e = tid; e < NB * NB; e += CB) {
        M[(long)(k0 + e / NB) * n + k0 + e % NB] = ds[e];
      }
    }
  }

  // pair = ti (ti + 1) / 2 + tj with tj <= ti.
  int ti = (int)((sqrtf(8.0f * pair + 1.0f) - 1.0f) * 0.5f);
  while (ti * (ti + 1) / 2 > pair) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= pair) ++ti;
  const int tj = pair - ti * (ti + 1) / 2;
  const int ib = k0 + NB + ti * TT;
  const int jb = k0 + NB + tj * TT;
  const int ty = tid / 16, tx = tid % 16;
  const int i0 = ib + 4 * ty, j0 = jb + 4 * tx;

  // All global loads first: the two 64 x 32 operand slices, then C.
  // Rows and columns past n are clamped; their products are not stored.
  float c[4][4];
  if (VEC) {
    float4 a4[2], b4[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int e = tid + s * CB;
      const int rr = e / 8, cq = e % 8;
      a4[s] = *reinterpret_cast<const float4*>(
          M + (long)min(ib + rr, n - 1) * n + k0 + 4 * cq);
      b4[s] = *reinterpret_cast<const float4*>(
          M + (long)min(jb + rr, n - 1) * n + k0 + 4 * cq);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const float4 v = *reinterpret_cast<const float4*>(
          M + (long)min(i0 + a, n - 1) * n + min(j0, n - 4));
      c[a][0] = v.x;
      c[a][1] = v.y;
      c[a][2] = v.z;
      c[a][3] = v.w;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int e = tid + s * CB;
      const int rr = e / 8, cq = e % 8;
      As[4 * cq][rr] = a4[s].x;
      As[4 * cq + 1][rr] = a4[s].y;
      As[4 * cq + 2][rr] = a4[s].z;
      As[4 * cq + 3][rr] = a4[s].w;
      Bs[4 * cq][rr] = b4[s].x;
      Bs[4 * cq + 1][rr] = b4[s].y;
      Bs[4 * cq + 2][rr] = b4[s].z;
      Bs[4 * cq + 3][rr] = b4[s].w;
    }
  } else {
    float a1[8], b1[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int e = tid + s * CB;
      const int rr = e / NB, cc = e % NB;
      a1[s] = M[(long)min(ib + rr, n - 1) * n + k0 + cc];
      b1[s] = M[(long)min(jb + rr, n - 1) * n + k0 + cc];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        c[a][b] = M[(long)min(i0 + a, n - 1) * n + min(j0 + b, n - 1)];
      }
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int e = tid + s * CB;
      As[e % NB][e / NB] = a1[s];
      Bs[e % NB][e / NB] = b1[s];
    }
  }
  __syncthreads();

  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0f;
  }
#pragma unroll 8
  for (int p = 0; p < NB; ++p) {
    const float4 av = *reinterpret_cast<const float4*>(&As[p][4 * ty]);
    const float4 bv = *reinterpret_cast<const float4*>(&Bs[p][4 * tx]);
    const float al[4] = {av.x, av.y, av.z, av.w};
    const float bl[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        acc[a][b] = fmaf(al[a], bl[b], acc[a][b]);
      }
    }
  }

  // Lower triangle only; whole float4 where the four columns are in it.
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = i0 + a;
    if (i >= n) break;
    float* dst = M + (long)i * n + j0;
    if (VEC && j0 + 3 <= i) {
      *reinterpret_cast<float4*>(dst) =
          make_float4(c[a][0] - acc[a][0], c[a][1] - acc[a][1],
                      c[a][2] - acc[a][2], c[a][3] - acc[a][3]);
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (j0 + b <= i) dst[b] = c[a][b] - acc[a][b];
      }
    }
  }
}

// What one round launches: the panel's row tiles and the trailing
// update's workgroups per matrix (v2: 64-column strips; v6: tile pairs).
struct PotrfRound {
  int panel_tiles;
  int trailing_wgs;
};

// `impl`, here and in module.cpp, is one of these two; nothing else exists.
enum { POTRF_V2 = 2, POTRF_V6 = 6 };

// Rows per panel workgroup.
extern "C" int batched_potrf_panel_rows(int impl) {
  return impl == POTRF_V6 ? PANEL_ROWS : CB;
}

static PotrfRound potrf_round(int n, int k0, int impl) {
  const int panel_rows = batched_potrf_panel_rows(impl);
  const int nb = (n - k0) < NB ? (n - k0) : NB;
  const int rows = n - (k0 + nb);
  PotrfRound s;
  s.panel_tiles = rows > 0 ? (rows + panel_rows - 1) / panel_rows : 1;
  const int t = (rows + TT - 1) / TT;
  s.trailing_wgs = impl == POTRF_V6 ? t * (t + 1) / 2 : t;
  return s;
}

// True iff some round of the v2 / v6 factorization of an n x n matrix runs
// more than one row tile, i.e. needs the (R, NB, NB) diagonal scratch.
extern "C" int batched_potrf_needs_scratch(int n, int impl) {
  return n - NB > batched_potrf_panel_rows(impl) ? 1 : 0;
}

// Round 0, the largest, as the launcher below runs it: {panel row tiles,
// trailing workgroups per matrix}.
extern "C" void batched_potrf_launch_shape(int n, int impl, int out[2]) {
  const PotrfRound s = potrf_round(n, 0, impl);
  out[0] = s.panel_tiles;
  out[1] = s.trailing_wgs;
}

// Factors (R, N, N) `A` in place. `dscratch` is (R, NB, NB), needed iff
// batched_potrf_needs_scratch(n, impl).
extern "C" void launch_batched_potrf(float* A, int* info, float* dscratch,
                                     int r, int n, int impl,
                                     hipStream_t stream) {
  const bool vec = n % 4 == 0 && reinterpret_cast<uintptr_t>(A) % 16 == 0;
  for (int k0 = 0; k0 < n; k0 += NB) {
    const PotrfRound s = potrf_round(n, k0, impl);
    // More than one row tile implies rows below the block, so the
    // trailing launch that moves the parked block into place follows.
    float* park = s.panel_tiles > 1 ? dscratch : nullptr;
    const dim3 panel_grid(r, s.panel_tiles);
    if (impl == POTRF_V2) {
      hipLaunchKernelGGL(batched_potrf_panel_kernel, panel_grid, dim3(CB),
                         0, stream, A, info, park, r, n, k0);
    } else if (vec) {
      hipLaunchKernelGGL(batched_potrf_panel_cols_kernel<true>, panel_grid,
                         dim3(PANEL_ROWS), 0, stream, A, info, park, n, k0);
    } else {
      hipLaunchKernelGGL(batched_potrf_panel_cols_kernel<false>, panel_grid,
                         dim3(PANEL_ROWS), 0, stream, A, info, park, n, k0);
    }
    if (s.trailing_wgs == 0) continue;
    if (impl == POTRF_V2) {
      hipLaunchKernelGGL(batched_potrf_trailing_kernel,
                         dim3(r, s.trailing_wgs), dim3(CB), 0, stream, A,
                         (const float*)park, r, n, k0);
    } else if (vec) {
      hipLaunchKernelGGL(batched_potrf_trailing_tiled_kernel<true>,
                         dim3(r * s.trailing_wgs), dim3(CB), 0, stream, A,
                         (const float*)park, n, k0, s.trailing_wgs);
    } else {
      hipLaunchKernelGGL(batched_potrf_trailing_tiled_kernel<false>,
                         dim3(r * s.trailing_wgs), dim3(CB), 0, stream, A,
                         (const float*)park, n, k0, s.trailing_wgs);
    }
  }
}

template <int RPT>
static void launch_trsv_pipe(const float* L, float* b, int r, int n,
                             hipStream_t stream) {
  const bool vec = n % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(L) % 16 == 0;
  if (vec) {
    hipLaunchKernelGGL((batched_trsv_lower_pipe_kernel<RPT, true>),
                       dim3(r), dim3(CB), 0, stream, L, b, r, n);
  } else {
    hipLaunchKernelGGL((batched_trsv_lower_pipe_kernel<RPT, false>),
                       dim3(r), dim3(CB), 0, stream, L, b, r, n);
  }
}

// variant 0: pipelined register-resident solve while the rows fit
// (N <= 256 * TRSV_PIPE_MAX_RPT = 1280), else the LDS-staged kernel.
// variant 1: the LDS-staged kernel.
extern "C" void launch_batched_trsv_lower(const float* L, float* b,
                                          int r, int n, int variant,
                                          hipStream_t stream) {
  const int rpt = (n + CB - 1) / CB;
  if (variant == 1 || rpt > TRSV_PIPE_MAX_RPT) {
    hipLaunchKernelGGL(batched_trsv_lower_kernel, dim3(r), dim3(CB), 0,
                       stream, L, b, r, n);
    return;
  }
  switch (rpt) {
    case 1: launch_trsv_pipe<1>(L, b, r, n, stream); break;
    case 2: launch_trsv_pipe<2>(L, b, r, n, stream); break;
    case 3: launch_trsv_pipe<3>(L, b, r, n, stream); break;
    case 4: launch_trsv_pipe<4>(L, b, r, n, stream); break;
    default: launch_trsv_pipe<5>(L, b, r, n, stream); break;
  }
}
