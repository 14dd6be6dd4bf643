// Batched Cholesky + forward substitution for the NLL line search
// (gfx950). MAGMA's batched spotf2 panels cost ~54 ms per suggest at
// the headline shape (16 x 1000 x 1000 per L-BFGS iteration,
// profiles/sweep_kernels_r2.txt) in ~5000 tiny kernel launches, and
// the (R, N, 1) triangular solves dispatch as SERIAL rocblas trsv
// calls (~170 us each). These kernels run one WORKGROUP per matrix:
// a right-looking blocked factorization (NB=32 panels staged in LDS,
// register-held L21 rows for the trailing update) and a
// wave-synchronous blocked forward substitution. Forward-only: the
// autograd value_and_grad path keeps torch's factorization; the
// line-search (torch.no_grad) calls these.
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
#include <cstdlib>

#include "common.h"

#define CB 256
#define NB 32

extern "C" __global__ __launch_bounds__(CB) void
batched_potrf_kernel(float* __restrict__ A,    // (R, N, N) in-place L
                     int* __restrict__ info,   // (R,)
                     int r_count, int n) {
  __shared__ float diag[NB][NB + 1];
  __shared__ float jpanel[64][NB];
  __shared__ int s_info;
  const int r = blockIdx.x;
  if (r >= r_count) return;
  float* M = A + (long)r * n * n;
  const int tid = threadIdx.x;
  if (tid == 0) s_info = 0;
  __syncthreads();

  for (int k0 = 0; k0 < n; k0 += NB) {
    const int nb = min(NB, n - k0);
    for (int e = tid; e < nb * nb; e += CB) {
      diag[e / nb][e % nb] = M[(long)(k0 + e / nb) * n + k0 + e % nb];
    }
    __syncthreads();
    // Unblocked factor of the diagonal block in LDS.
    for (int j = 0; j < nb; ++j) {
      if (tid == 0) {
        const float v = diag[j][j];
        if (v > 0.0f) {
          diag[j][j] = sqrtf(v);
        } else {
          diag[j][j] = 1.0f;  // keep going; info marks the failure
          if (s_info == 0) s_info = k0 + j + 1;
        }
      }
      __syncthreads();
      const float dj = diag[j][j];
      for (int i = j + 1 + tid; i < nb; i += CB) {
        diag[i][j] /= dj;
      }
      __syncthreads();
      const int rem = nb - j - 1;
      for (int e = tid; e < rem * rem; e += CB) {
        const int i = j + 1 + e / rem;
        const int c = j + 1 + e % rem;
        if (c <= i) diag[i][c] -= diag[i][j] * diag[c][j];
      }
      __syncthreads();
    }
    for (int e = tid; e < nb * nb; e += CB) {
      const int i = e / nb, c = e % nb;
      M[(long)(k0 + i) * n + k0 + c] = (c <= i) ? diag[i][c] : 0.0f;
    }
    __syncthreads();

    // Column panel: L21 = A21 * L11^-T, one row per thread.
    for (int i = k0 + nb + tid; i < n; i += CB) {
      float v[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        if (j < nb) {
          float xv = M[(long)i * n + k0 + j];
#pragma unroll
          for (int p = 0; p < NB; ++p) {
            if (p < j) xv -= v[p] * diag[j][p];
          }
          v[j] = xv / diag[j][j];
        }
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        if (j < nb) M[(long)i * n + k0 + j] = v[j];
      }
    }
    __syncthreads();

    // Trailing update (lower triangle only): A22 -= L21 L21^T.
    for (int jb = k0 + nb; jb < n; jb += 64) {
      const int jl = min(64, n - jb);
      for (int e = tid; e < jl * nb; e += CB) {
        jpanel[e / nb][e % nb] = M[(long)(jb + e / nb) * n + k0 + e % nb];
      }
      __syncthreads();
      for (int i = jb + tid; i < n; i += CB) {
        float row[NB];
#pragma unroll
        for (int p = 0; p < NB; ++p) {
          row[p] = (p < nb) ? M[(long)i * n + k0 + p] : 0.0f;
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
  if (tid == 0) info[r] = s_info;
}

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

// -- v2: panel-swept factorization --------------------------------------
//
// v1 (one workgroup per matrix for the WHOLE factorization) measured
// slower than MAGMA in context: at batch 16 only 16 CUs work and the
// trailing updates serialize inside each workgroup. v2 keeps the
// panel factor per-matrix (small) but launches the trailing update as
// a (R x column-tiles) grid per panel — 2 launches per panel (~64
// total) with the O(N^2) trailing work spread over the chip.

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

// -- v3: persistent cooperative factorization (OPT-IN, measured slower)
//
// One cooperative launch for all panels with eagle_sweep-style grid
// barriers, pair (r, t) owning 64-row tile t. MEASURED RESULT at the
// headline shape: warm refit 132.9 -> 240.9 ms — SLOWER than v2's 64
// dependent launches. Root cause: a right-looking factorization
// rewrites the whole trailing matrix every round, and cross-workgroup
// coherence inside one kernel forces those reads+writes through
// agent-scope (memory-side, uncached) accesses — ~1.3 GB of L2-bypass
// traffic per N=1000 factorization, which costs more than the launch
// turnarounds it saves. (eagle_sweep wins with this pattern because
// its bulk data — K^-1, x, alpha — is READ-ONLY and stays L2-cached;
// only small buffers cross workgroups.) Kept opt-in
// (VIZIER_AMD_COOP_CHOL=1) as a documented experiment.

__device__ __forceinline__ float cchol_load(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cchol_store(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int cchol_iload(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cchol_istore(int* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void chol_grid_sync(unsigned int* bar) {
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int gen =
        __hip_atomic_load(bar + 1, __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("" ::: "memory");
    const unsigned int arrived = __hip_atomic_fetch_add(
        bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (arrived == gridDim.x - 1) {
      __hip_atomic_store(bar, 0u, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_s_waitcnt(0);
      __hip_atomic_fetch_add(bar + 1, 1u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    } else {
      while (__hip_atomic_load(bar + 1, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT) == gen) {
        __builtin_amdgcn_s_sleep(8);
      }
    }
    asm volatile("" ::: "memory");
  }
  __syncthreads();
}

#define RB 64  // rows per ownership tile

extern "C" __global__ __launch_bounds__(CB) void
batched_potrf_coop_kernel(float* __restrict__ A, int* __restrict__ info,
                          unsigned int* __restrict__ bar,
                          int r_count, int n) {
  __shared__ float diag[NB][NB + 1];
  __shared__ float myl[RB][NB];
  __shared__ float jpanel[RB][NB];
  const int tid = threadIdx.x;
  const int tiles = (n + RB - 1) / RB;
  const int npairs = r_count * tiles;

  for (int k0 = 0; k0 < n; k0 += NB) {
    const int nb = min(NB, n - k0);
    // Phase A/B: redundant diagonal factor + owned panel rows. The
    // factored diagonal is NOT written back here — every pair reads
    // the ORIGINAL diag values, so a writeback would race with other
    // pairs' loads. The owner writes it in phase C (whose trailing
    // updates touch disjoint rows) after a cheap redundant re-factor.
    for (int pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
      const int r = pair / tiles, t = pair % tiles;
      const int tile_lo = t * RB;
      const int tile_hi = min(tile_lo + RB, n);
      if (tile_hi <= k0 + nb) continue;  // no panel rows in this tile
      float* M = A + (long)r * n * n;
      if (tid < WAVE_SIZE) {
        const int lane = tid;
        float row[NB];
#pragma unroll
        for (int c = 0; c < NB; ++c) {
          row[c] = (lane < nb && c < nb)
              ? cchol_load(&M[(long)(k0 + lane) * n + k0 + c]) : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          if (j >= nb) break;
          const float piv = __shfl(row[j], j, WAVE_SIZE);
          const float d = (piv > 0.0f) ? sqrtf(piv) : 1.0f;
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
      const int row_lo = max(tile_lo, k0 + nb);
      const int i = row_lo + tid;  // one row per thread (<= 64 rows)
      if (i < tile_hi) {
        float v[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          if (j < nb) {
            float xv = cchol_load(&M[(long)i * n + k0 + j]);
#pragma unroll
            for (int p = 0; p < NB; ++p) {
              if (p < j) xv -= v[p] * diag[j][p];
            }
            v[j] = xv / diag[j][j];
          }
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          if (j < nb) cchol_store(&M[(long)i * n + k0 + j], v[j]);
        }
      }
      __syncthreads();  // diag LDS reused by the next pair
    }
    chol_grid_sync(bar);

    // Phase C: owner writes the factored diagonal (re-factored from
    // the still-original values — trailing writes touch disjoint
    // rows), then the trailing update of owned rows (identical fma
    // chains to batched_potrf_trailing_kernel).
    for (int pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
      const int r = pair / tiles, t = pair % tiles;
      const int tile_lo = t * RB;
      const int tile_hi = min(tile_lo + RB, n);
      float* M = A + (long)r * n * n;
      if (t == k0 / RB) {
        if (tid < WAVE_SIZE) {
          const int lane = tid;
          float row[NB];
#pragma unroll
          for (int c = 0; c < NB; ++c) {
            row[c] = (lane < nb && c < nb)
                ? cchol_load(&M[(long)(k0 + lane) * n + k0 + c]) : 0.0f;
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
              if (lane == 0 && cchol_iload(&info[r]) == 0) {
                cchol_istore(&info[r], k0 + j + 1);
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
        for (int e = tid; e < nb * nb; e += CB) {
          const int i = e / nb, c = e % nb;
          cchol_store(&M[(long)(k0 + i) * n + k0 + c],
                      (c <= i) ? diag[i][c] : 0.0f);
        }
        __syncthreads();
      }
      const int row_lo = max(tile_lo, k0 + nb);
      if (row_lo >= tile_hi) continue;
      const int nrows = tile_hi - row_lo;
      for (int e = tid; e < nrows * nb; e += CB) {
        myl[e / nb][e % nb] =
            cchol_load(&M[(long)(row_lo + e / nb) * n + k0 + e % nb]);
      }
      __syncthreads();
      for (int jb = k0 + nb; jb < tile_hi; jb += RB) {
        const int jl = min(RB, n - jb);
        for (int e = tid; e < jl * nb; e += CB) {
          jpanel[e / nb][e % nb] =
              cchol_load(&M[(long)(jb + e / nb) * n + k0 + e % nb]);
        }
        __syncthreads();
        const int rl = tid >> 2, jq = tid & 3;
        const int i = row_lo + rl;
        if (rl < nrows && i >= jb) {
          for (int q = 0; q < 16; ++q) {
            const int j = jq * 16 + q;
            if (j < jl && jb + j <= i) {
              float acc = 0.0f;
#pragma unroll
              for (int p = 0; p < NB; ++p) {
                acc = fmaf(myl[rl][p], jpanel[j][p], acc);
              }
              float* dst = &M[(long)i * n + jb + j];
              cchol_store(dst, cchol_load(dst) - acc);
            }
          }
        }
        __syncthreads();
      }
    }
    chol_grid_sync(bar);
  }
}

extern "C" int launch_batched_potrf_coop(float* A, int* info,
                                         unsigned int* bar, int r, int n,
                                         hipStream_t stream) {
  int max_blocks = 0;
  hipError_t err = hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &max_blocks, (const void*)batched_potrf_coop_kernel, CB, 0);
  if (err != hipSuccess || max_blocks < 1) return -1;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return -1;
  const int tiles = (n + RB - 1) / RB;
  int grid = r * tiles;
  const int cap = max_blocks * prop.multiProcessorCount;
  if (grid > cap) grid = cap;
  if (grid < 1) grid = 1;
  void* args[] = {&A, &info, &bar, &r, &n};
  err = hipLaunchCooperativeKernel(
      (const void*)batched_potrf_coop_kernel, dim3(grid), dim3(CB),
      args, 0, stream);
  return err == hipSuccess ? 0 : -1;
}

// -- v4: fused round kernel (default) -----------------------------------
//
// ONE launch per 32-panel round instead of v2's two (panel + trailing),
// with NO cross-workgroup coherence traffic: round k's kernel never
// writes anything another workgroup of the same launch reads. The
// trick is write deferral + recomputation:
//   - the factored 32x32 diagonal stays OUT of A until the final
//     cleanup kernel (each consumer re-factors it from A's stable
//     values in-wave — ~1 us, deterministic);
//   - L21 panel rows are recomputed from A's original column values by
//     every workgroup that needs them (solve vs the LDS diagonal), and
//     only written back for round k-1 (whose columns nothing in round
//     k reads);
//   - the trailing update is in-place on disjoint (i, j >= jb) tiles.
// Per-element fma chains are IDENTICAL to v2, so v4 results are
// bit-identical to v2's. What motivated it was potrf R=3 == R=12 ==
// 2.85 ms on v2, read then as a ~44 us launch + L2-flush turnaround
// BETWEEN dependent kernels. That reading was wrong: the time is the
// serial chain inside v2's critical workgroups, which is why halving the
// launches did not help (113 us per round here) and why v6, with v2's
// launch count, takes 0.63 ms (see the v6 header).

__device__ __forceinline__ void wave_factor_diag(
    const float* __restrict__ M, int n, int k0, int nb,
    float diag_out[NB][NB + 1], int* fail_col /* -1 if ok */) {
  const int lane = threadIdx.x;
  float row[NB];
  int fc = -1;
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
      if (fc < 0) fc = k0 + j + 1;
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
    if (lane < nb && c < nb) diag_out[lane][c] = row[c];
  }
  *fail_col = fc;
}

__device__ __forceinline__ void solve_panel_row(
    const float* __restrict__ M, int n, int i, int k0, int nb,
    const float diag[NB][NB + 1], float v[NB]) {
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    if (j < nb) {
      float xv = M[(long)i * n + k0 + j];
#pragma unroll
      for (int p = 0; p < NB; ++p) {
        if (p < j) xv -= v[p] * diag[j][p];
      }
      v[j] = xv / diag[j][j];
    }
  }
}

extern "C" __global__ __launch_bounds__(CB) void
batched_potrf_round_kernel(float* __restrict__ A, int* __restrict__ info,
                           int r_count, int n, int k0) {
  __shared__ float pdiag[NB][NB + 1];  // factored diag of round k-1
  __shared__ float diag[NB][NB + 1];   // factored diag of round k
  __shared__ float jpanel[64][NB];     // L21^k rows of this j-tile
  const int r = blockIdx.x;
  if (r >= r_count) return;
  float* M = A + (long)r * n * n;
  const int tid = threadIdx.x;
  const int nb = min(NB, n - k0);
  const int k0p = k0 - NB;

  // Step 0: finalize round k-1 — write L21^{k-1} for this tile's rows
  // (columns k0p, which nothing in round k reads).
  if (k0p >= 0) {
    int fcp = -1;
    if (tid < WAVE_SIZE) {
      wave_factor_diag(M, n, k0p, NB, pdiag, &fcp);
    }
    __syncthreads();
    if (blockIdx.y == 0 && tid == 0 && fcp > 0 && info[r] == 0) {
      info[r] = fcp;  // unique writer per launch; launches are ordered
    }
    const int w0 = k0 + (int)blockIdx.y * 64;
    for (int i = w0 + tid; i < min(w0 + 64, n); i += CB) {
      float v[NB];
      solve_panel_row(M, n, i, k0p, NB, pdiag, v);
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        M[(long)i * n + k0p + j] = v[j];
      }
    }
  }

  // Step 1: trailing update for this j-tile (jb >= k0+nb), using L21^k
  // recomputed from A's still-original panel columns.
  const int jb = k0 + nb + (int)blockIdx.y * 64;
  if (jb >= n || nb < NB) return;  // last round has no trailing
  int fc = -1;
  if (tid < WAVE_SIZE) {
    wave_factor_diag(M, n, k0, nb, diag, &fc);
  }
  __syncthreads();
  const int jl = min(64, n - jb);
  // Recompute L21 rows of this j-tile into LDS (identical solve chain).
  for (int j = tid; j < jl; j += CB) {
    float v[NB];
    solve_panel_row(M, n, jb + j, k0, nb, diag, v);
#pragma unroll
    for (int p = 0; p < NB; ++p) jpanel[j][p] = v[p];
  }
  __syncthreads();
  for (int i = jb + tid; i < n; i += CB) {
    float v[NB];
    solve_panel_row(M, n, i, k0, nb, diag, v);
    for (int j = 0; j < jl; ++j) {
      if (jb + j > i) break;
      float acc = 0.0f;
#pragma unroll
      for (int p = 0; p < NB; ++p) {
        acc = fmaf(v[p], jpanel[j][p], acc);
      }
      M[(long)i * n + jb + j] -= acc;
    }
  }
}

// Final cleanup: factor every diagonal block in place (their inputs
// are stable once the preceding trailing rounds ran), zero the upper
// part, and record a failure in the LAST block (earlier blocks were
// recorded by their successor round's step 0).
extern "C" __global__ __launch_bounds__(CB) void
batched_potrf_final_kernel(float* __restrict__ A, int* __restrict__ info,
                           int r_count, int n) {
  __shared__ float diag[NB][NB + 1];
  const int r = blockIdx.x;
  if (r >= r_count) return;
  float* M = A + (long)r * n * n;
  const int tid = threadIdx.x;
  const int k0 = (int)blockIdx.y * NB;
  const int nb = min(NB, n - k0);
  int fc = -1;
  if (tid < WAVE_SIZE) {
    wave_factor_diag(M, n, k0, nb, diag, &fc);
  }
  __syncthreads();
  if (tid == 0 && fc > 0 && k0 + NB >= n && info[r] == 0) {
    info[r] = fc;
  }
  for (int e = tid; e < nb * nb; e += CB) {
    const int i = e / nb, c = e % nb;
    M[(long)(k0 + i) * n + k0 + c] = (c <= i) ? diag[i][c] : 0.0f;
  }
}

// -- v5: persistent LEFT-looking cooperative factorization --------------
//
// Why a 5th design: the per-kernel cost of v2's 63 launches is NOT
// launch overhead (a 63-deep chain of trivial kernels runs at 4.4
// us/launch) and NOT uncoalesced access (LDS staging changed nothing).
// It was put down to an end-of-kernel release fence writing back and
// invalidating the per-XCD L2s (~40-65 us), and v5 was built to run the
// whole factorization in ONE kernel with the bulk data CACHED, which a
// right-looking update cannot do (v3: the trailing matrix is
// cross-workgroup mutable). The premise does not hold: v6 keeps all 63
// kernel boundaries and the same dirty bytes and runs in 0.63 ms, so a
// boundary costs microseconds and v2's time is inside its kernels.
//
// Left-looking solves it:
//   - the INPUT matrix A is never written (output is separate), so
//     its reads are normal cached loads;
//   - finalized L panels live in a PANEL-MAJOR scratch (32 floats per
//     row per panel, 128-byte aligned) so no cache line ever spans
//     two panels; a line is cstore'd once at finalization and only
//     normal-loaded AFTER that, so caches can never hold a stale
//     pre-write copy;
//   - only the factored 32x32 diagonal block crosses workgroups
//     mid-round, through a tiny agent-scope scratch.
// A plain kernel afterwards copies panel-major L into the dense
// output with the upper triangle zeroed.
//
// Round k, pair (r, t) owning 64-row tile t (one pair per workgroup,
// enforced by the launcher):
//   P1: rows_acc[i][c] = A[i, k0+c] - sum_{kb<k} L[i,:] L[k0+c,:]
//       (4 threads x 8 columns per row; LDS-staged L tiles);
//       the diagonal owner wave-factors rows_acc, records info, and
//       publishes the factored diagonal via agent-scope scratch.
//   barrier.
//   P2: every tile solves its own rows >= k0+32 against the diagonal
//       and finalizes them into the panel scratch.
//   barrier.

#define V5_RB 64

extern "C" __global__ __launch_bounds__(CB) void
batched_potrf_left_kernel(
    const float* __restrict__ A,     // (R, N, N) input, read-only
    float* __restrict__ panels,      // (R, ceil(N/32), N, 32) scratch
    float* __restrict__ dscratch,    // (R, 32, 32) diag broadcast
    int* __restrict__ info,          // (R,)
    unsigned int* __restrict__ bar,  // (2,) zeroed
    int r_count, int n) {
  __shared__ float rows_acc[V5_RB][NB + 1];
  __shared__ float lrows[V5_RB][NB];   // own-tile L rows, one kb panel
  __shared__ float ldiag[NB][NB + 1];  // diag-rows L, one kb panel
  __shared__ float fdiag[NB][NB + 1];  // factored diagonal this round
  const int tid = threadIdx.x;
  const int tiles = (n + V5_RB - 1) / V5_RB;
  const int r = blockIdx.x / tiles;
  const int t = blockIdx.x % tiles;
  const int tile_lo = t * V5_RB;
  const int tile_hi = min(tile_lo + V5_RB, n);
  const float* Ain = A + (long)r * n * n;
  float* P = panels + (long)r * ((n + NB - 1) / NB) * n * NB;
  float* ds = dscratch + (long)r * NB * NB;
  const int n_rounds = (n + NB - 1) / NB;

  for (int k = 0; k < n_rounds; ++k) {
    const int k0 = k * NB;
    const int nb = min(NB, n - k0);
    const int row_lo = tile_lo > k0 ? tile_lo : k0;
    const bool active = tile_hi > k0;
    const bool owner = (k0 >= tile_lo && k0 < tile_hi);

    if (active) {
      // P1: update own rows' panel columns (left-looking GEMM).
      const int nrows = tile_hi - row_lo;
      const int rl = tid >> 2, cq = (tid & 3) * 8;
      float acc[8];
      const int i = row_lo + rl;
      if (rl < nrows) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          acc[c] = (cq + c < nb) ? Ain[(long)i * n + k0 + cq + c] : 0.0f;
        }
      }
      for (int kb = 0; kb < k; ++kb) {
        const float* Pk = P + (long)kb * n * NB;
        for (int e = tid; e < nrows * NB; e += CB) {
          lrows[e / NB][e % NB] = Pk[(long)(row_lo + e / NB) * NB
                                     + e % NB];
        }
        for (int e = tid; e < nb * NB; e += CB) {
          ldiag[e / NB][e % NB] = Pk[(long)(k0 + e / NB) * NB + e % NB];
        }
        __syncthreads();
        if (rl < nrows) {
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            float a = acc[c];
            if (cq + c < nb) {
#pragma unroll
              for (int p = 0; p < NB; ++p) {
                a = fmaf(-lrows[rl][p], ldiag[cq + c][p], a);
              }
            }
            acc[c] = a;
          }
        }
        __syncthreads();
      }
      if (rl < nrows) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          rows_acc[rl][cq + c] = acc[c];
        }
      }
      __syncthreads();

      if (owner) {
        // Wave-factor the updated diagonal block (rows k0..k0+nb are
        // inside this tile) and publish it.
        const int d0 = k0 - row_lo;
        int fc = -1;
        if (tid < WAVE_SIZE) {
          const int lane = tid;
          float row[NB];
#pragma unroll
          for (int c = 0; c < NB; ++c) {
            row[c] = (lane < nb && c < nb) ? rows_acc[d0 + lane][c]
                                           : 0.0f;
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
              if (fc < 0) fc = k0 + j + 1;
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
            if (lane < nb && c < nb) fdiag[lane][c] = row[c];
          }
          if (lane == 0 && fc > 0 && cchol_iload(&info[r]) == 0) {
            cchol_istore(&info[r], fc);
          }
        }
        __syncthreads();
        // Publish diag: agent-scope scratch for other tiles + the
        // finalized panel rows for later rounds' GEMMs.
        float* Pk = P + (long)k * n * NB;
        for (int e = tid; e < nb * nb; e += CB) {
          const int ii = e / nb, c = e % nb;
          cchol_store(&ds[ii * NB + c], fdiag[ii][c]);
          cchol_store(&Pk[(long)(k0 + ii) * NB + c],
                      (c <= ii) ? fdiag[ii][c] : 0.0f);
        }
      }
    }
    chol_grid_sync(bar);

    // P2: solve own rows below the diagonal block and finalize them.
    if (active) {
      const int row_lo2 = tile_lo > k0 + nb ? tile_lo : k0 + nb;
      if (row_lo2 < tile_hi) {
        if (!owner) {
          for (int e = tid; e < nb * nb; e += CB) {
            fdiag[e / nb][e % nb] = cchol_load(&ds[(e / nb) * NB
                                                   + e % nb]);
          }
        }
        __syncthreads();
        const int base = row_lo2 - (tile_lo > k0 ? tile_lo : k0);
        const int i = row_lo2 + tid;
        float* Pk = P + (long)k * n * NB;
        if (i < tile_hi) {
          float v[NB];
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            if (j < nb) {
              float xv = rows_acc[base + tid][j];
#pragma unroll
              for (int p = 0; p < NB; ++p) {
                if (p < j) xv -= v[p] * fdiag[j][p];
              }
              v[j] = xv / fdiag[j][j];
            } else {
              v[j] = 0.0f;
            }
          }
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            cchol_store(&Pk[(long)i * NB + j], v[j]);
          }
        }
      }
      __syncthreads();
    }
    chol_grid_sync(bar);
  }
}

// Copies panel-major L into the dense (R, N, N) output, zeroing the
// upper triangle (and the never-written rows above each panel).
extern "C" __global__ __launch_bounds__(CB) void
potrf_copy_out_kernel(const float* __restrict__ panels,
                      float* __restrict__ L, int r_count, int n) {
  const int r = blockIdx.x;
  if (r >= r_count) return;
  const int pk = blockIdx.y;
  const int p0 = pk * NB;
  const float* Pk = panels + ((long)r * ((n + NB - 1) / NB) + pk)
                    * (long)n * NB;
  float* M = L + (long)r * n * n;
  for (int e = threadIdx.x; e < n * NB; e += CB) {
    const int i = e / NB, p = e % NB;
    const int j = p0 + p;
    if (j < n) {
      M[(long)i * n + j] = (j <= i) ? Pk[(long)i * NB + p] : 0.0f;
    }
  }
}

extern "C" int launch_batched_potrf_v5(const float* A, float* panels,
                                       float* dscratch, float* L,
                                       int* info, unsigned int* bar,
                                       int r, int n,
                                       hipStream_t stream) {
  int max_blocks = 0;
  hipError_t err = hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &max_blocks, (const void*)batched_potrf_left_kernel, CB, 0);
  if (err != hipSuccess || max_blocks < 1) return -1;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return -1;
  const int tiles = (n + V5_RB - 1) / V5_RB;
  const int grid = r * tiles;
  if (grid > max_blocks * prop.multiProcessorCount) return -1;
  void* args[] = {&A, &panels, &dscratch, &info, &bar, &r, &n};
  err = hipLaunchCooperativeKernel(
      (const void*)batched_potrf_left_kernel, dim3(grid), dim3(CB),
      args, 0, stream);
  if (err != hipSuccess) return -1;
  const int pk = (n + NB - 1) / NB;
  hipLaunchKernelGGL(potrf_copy_out_kernel, dim3(r, pk), dim3(CB), 0,
                     stream, panels, L, r, n);
  return 0;
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

// Rows per panel workgroup of the v2 (impl != 6) and v6 launchers.
extern "C" int batched_potrf_panel_rows(int impl) {
  return impl == 6 ? PANEL_ROWS : CB;
}

static PotrfRound potrf_round(int n, int k0, int impl) {
  const int panel_rows = batched_potrf_panel_rows(impl);
  const int nb = (n - k0) < NB ? (n - k0) : NB;
  const int rows = n - (k0 + nb);
  PotrfRound s;
  s.panel_tiles = rows > 0 ? (rows + panel_rows - 1) / panel_rows : 1;
  const int t = (rows + TT - 1) / TT;
  s.trailing_wgs = impl == 6 ? t * (t + 1) / 2 : t;
  return s;
}

// True iff some round of the v2 / v6 factorization of an n x n matrix runs
// more than one row tile, i.e. needs the (R, NB, NB) diagonal scratch.
extern "C" int batched_potrf_needs_scratch(int n, int impl) {
  return n - NB > batched_potrf_panel_rows(impl) ? 1 : 0;
}

// Round 0, the largest, as the launchers below run it: {panel row tiles,
// trailing workgroups per matrix}.
extern "C" void batched_potrf_launch_shape(int n, int impl, int out[2]) {
  const PotrfRound s = potrf_round(n, 0, impl);
  out[0] = s.panel_tiles;
  out[1] = s.trailing_wgs;
}

extern "C" void launch_batched_potrf_v6(float* A, int* info,
                                        float* dscratch, int r, int n,
                                        hipStream_t stream) {
  const bool vec = n % 4 == 0 && reinterpret_cast<uintptr_t>(A) % 16 == 0;
  for (int k0 = 0; k0 < n; k0 += NB) {
    const PotrfRound s = potrf_round(n, k0, 6);
    // More than one row tile implies rows below the block, so the
    // trailing launch that moves the parked block into place follows.
    float* park = s.panel_tiles > 1 ? dscratch : nullptr;
    if (vec) {
      hipLaunchKernelGGL(batched_potrf_panel_cols_kernel<true>,
                         dim3(r, s.panel_tiles), dim3(PANEL_ROWS), 0,
                         stream, A, info, park, n, k0);
    } else {
      hipLaunchKernelGGL(batched_potrf_panel_cols_kernel<false>,
                         dim3(r, s.panel_tiles), dim3(PANEL_ROWS), 0,
                         stream, A, info, park, n, k0);
    }
    if (s.trailing_wgs > 0) {
      if (vec) {
        hipLaunchKernelGGL(batched_potrf_trailing_tiled_kernel<true>,
                           dim3(r * s.trailing_wgs), dim3(CB), 0, stream,
                           A, (const float*)park, n, k0, s.trailing_wgs);
      } else {
        hipLaunchKernelGGL(batched_potrf_trailing_tiled_kernel<false>,
                           dim3(r * s.trailing_wgs), dim3(CB), 0, stream,
                           A, (const float*)park, n, k0, s.trailing_wgs);
      }
    }
  }
}

extern "C" void launch_batched_potrf_v2(float* A, int* info,
                                        float* dscratch, int r, int n,
                                        hipStream_t stream) {
  for (int k0 = 0; k0 < n; k0 += NB) {
    const int nb = (n - k0) < NB ? (n - k0) : NB;
    const int rows = n - (k0 + nb);
    const int rtiles = rows > 0 ? (rows + CB - 1) / CB : 1;
    // rtiles > 1 implies rows > CB, so the trailing launch that moves
    // the parked block into place always follows.
    float* park = rtiles > 1 ? dscratch : nullptr;
    hipLaunchKernelGGL(batched_potrf_panel_kernel, dim3(r, rtiles),
                       dim3(CB), 0, stream, A, info, park, r, n, k0);
    const int jtiles = (rows + 63) / 64;
    if (jtiles > 0) {
      hipLaunchKernelGGL(batched_potrf_trailing_kernel,
                         dim3(r, jtiles), dim3(CB), 0, stream, A,
                         (const float*)park, r, n, k0);
    }
  }
}

// impl: 6 = v6, 4 = v4, else v2. v4 measured SLOWER than v2 at the headline shape (3.63
// vs 2.85 ms, R=3 N=1000): the fused kernel's three inlined 32-wide solves
// blow its register budget (VGPR 256 + 248 AGPRs, occupancy 1 wave/SIMD
// vs v2's 4). Kept for experiments.
extern "C" void launch_batched_potrf(float* A, int* info, float* dscratch,
                                     int r, int n, int impl,
                                     hipStream_t stream) {
  if (impl == 6) {
    launch_batched_potrf_v6(A, info, dscratch, r, n, stream);
    return;
  }
  if (impl != 4) {
    launch_batched_potrf_v2(A, info, dscratch, r, n, stream);
    return;
  }
  for (int k0 = 0; k0 < n; k0 += NB) {
    const int nb = (n - k0) < NB ? (n - k0) : NB;
    const int step0_tiles = (n - k0 + 63) / 64;
    const int jtiles = (n - (k0 + nb) + 63) / 64;
    int tiles = step0_tiles > jtiles ? step0_tiles : jtiles;
    if (tiles < 1) tiles = 1;
    if (k0 == 0 && jtiles == 0) break;  // single block: final only
    hipLaunchKernelGGL(batched_potrf_round_kernel, dim3(r, tiles),
                       dim3(CB), 0, stream, A, info, r, n, k0);
  }
  const int blocks = (n + NB - 1) / NB;
  hipLaunchKernelGGL(batched_potrf_final_kernel, dim3(r, blocks),
                     dim3(CB), 0, stream, A, info, r, n);
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
