// Device helpers shared by the persistent sweep megakernels:
// eagle_sweep.hip (continuous spaces), eagle_sweep_mixed.hip (mixed
// categorical + continuous spaces) and eagle_sweep_mo.hip (several metrics,
// continuous spaces). The kernels have the same workgroup
// shape, the same grid barrier, the same block reductions and the same
// 64x64 tile quadform, so their phases B / B2 and the reduce of C / RC are
// one text. See the header of eagle_sweep.hip for the design.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

// The workgroup has SWEEP_THREADS threads: two halves of BLOCK. Phase B
// runs one tile per half; every other phase is the BLOCK-thread arithmetic
// of the step kernels on half 0 (waves 0..3), with half 1 predicated off.
#define BLOCK 256
#define SWEEP_THREADS (2 * BLOCK)
// Loop start of a half-1 thread in the BLOCK-thread phases: past every
// bound (all are below 2^24), and + 4 * BLOCK does not overflow.
#define SWEEP_IDLE (1 << 30)
#define MAX_POOL 128
#define SWEEP_NCHUNK 10   // must match posterior_score.hip's NCHUNK
#define POOL_LDS_CAP 8192  // floats: stage pool in LDS when it fits
// floats: at or below this the pool lives in the upper half of pool_lds
// for the whole launch (phase B stages k_i / k_j in the lower half only).
#define RESIDENT_CAP (POOL_LDS_CAP / 2)
// Categorical entries (pool_size * dcat) the mixed kernel keeps in LDS as
// 16-bit indices beside the continuous pool: 6144 bytes, which with its
// four 512-entry parameter tables (4096 bytes) takes the kernel's static
// LDS from 52,792 to 63,032 of the 65,536 bytes a kernel may declare.
#define RESIDENT_CAT_CAP 3072

// Agent-scope (device) coherent access helpers: compile to memory-side
// accesses that bypass the incoherent per-XCD L2 path for plain loads.
__device__ __forceinline__ float cload(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cstore(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Grid barrier on ONE agent-scope counter that only grows. bar[0] counts
// arrivals over the whole launch and is zeroed by the caller before every
// launch; bar[1] is unused. The k-th barrier of the launch (k = 0, 1, ...)
// is complete once bar[0] >= (k + 1) * G. Every workgroup keeps
// `target` = (k + 1) * G in a register and advances it identically, so a
// barrier is one fetch_add plus polls of the same word: two dependent
// memory-side round trips, where the sense-reversing form it replaced took
// about five (generation load, fetch_add, reset store, waitcnt,
// generation fetch_add, then the pollers' load). A fast workgroup that
// arrives at barrier k + 1 while a slow one still polls barrier k only
// pushes the count further past the slow one's target, and the count
// cannot reach (k + 2) * G before everyone has arrived at k + 1. The
// compare is on the signed difference, so wrap-around of the counter is
// harmless.
//
// Deliberately RELAXED atomics: acq_rel orderings compile to
// buffer_wbl2 / buffer_inv (full per-XCD L2 writeback+invalidate),
// which costs tens of microseconds per barrier AND evicts the
// L2-resident K^-1 that phase B depends on. Ordering is instead
// established by hand:
//   - every thread drains its own outstanding global ops
//     (s_waitcnt 0) before the block barrier, so all sc1 data stores
//     have reached the coherence point before tid 0 arrives;
//   - all cross-workgroup data moves through sc1 accesses (cload /
//     cstore), which always read/write the coherence point, so no
//     cache invalidation is needed on the acquire side;
//   - waves issue memory ops in order, so the spin-exit load ordering
//     is sufficient (compiler reordering is fenced with asm).
__device__ __forceinline__ void grid_sync(unsigned int* bar,
                                          unsigned int& target) {
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  target += gridDim.x;
  if (threadIdx.x == 0) {
    asm volatile("" ::: "memory");
    // The value the fetch_add returns already tells the last arriver
    // that the barrier is complete.
    const unsigned int count = __hip_atomic_fetch_add(
        bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
    if ((int)(count - target) < 0) {
      while ((int)(__hip_atomic_load(bar, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT) -
                   target) < 0) {
        __builtin_amdgcn_s_sleep(8);
      }
    }
    asm volatile("" ::: "memory");
  }
  __syncthreads();
}

// block_reduce (common.h) for the sweep's eight-wave workgroup: the shuffle
// tree per wave, then the 4-lane second stage over waves 0..3 only, in
// block_reduce's order for a 256-thread block. Waves 4..7 run the shuffles
// on a value nobody reads, store nothing (lds4[4..6] hold other scalars)
// and take the __syncthreads. Result valid in thread 0.
template <typename T, typename Op>
__device__ __forceinline__ T sweep_block_reduce(T v, T* lds4, Op op,
                                                T init) {
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
#pragma unroll
  for (int offset = WAVE_SIZE / 2; offset > 0; offset >>= 1) {
    v = op(v, __shfl_down(v, offset, WAVE_SIZE));
  }
  if (lane == 0 && wave < BLOCK / WAVE_SIZE) lds4[wave] = v;
  __syncthreads();
  if (wave == 0) {
    v = (lane < BLOCK / WAVE_SIZE) ? lds4[lane] : init;
#pragma unroll
    for (int offset = 2; offset > 0; offset >>= 1) {
      v = op(v, __shfl_down(v, offset, WAVE_SIZE));
    }
  }
  return v;
}

// Two reductions on one barrier pass: each value goes through
// sweep_block_reduce's shuffles and second stage on its own, with its own
// LDS slots, so each result has the bits of a reduction of its own; only
// the __syncthreads is shared. Results in place, valid in thread 0.
template <typename T, typename Op1, typename Op2>
__device__ __forceinline__ void sweep_block_reduce2(
    T& v1, T& v2, T* lds4a, T* lds4b, Op1 op1, Op2 op2, T init1, T init2) {
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
#pragma unroll
  for (int offset = WAVE_SIZE / 2; offset > 0; offset >>= 1) {
    v1 = op1(v1, __shfl_down(v1, offset, WAVE_SIZE));
    v2 = op2(v2, __shfl_down(v2, offset, WAVE_SIZE));
  }
  if (lane == 0 && wave < BLOCK / WAVE_SIZE) {
    lds4a[wave] = v1;
    lds4b[wave] = v2;
  }
  __syncthreads();
  if (wave == 0) {
    v1 = (lane < BLOCK / WAVE_SIZE) ? lds4a[lane] : init1;
    v2 = (lane < BLOCK / WAVE_SIZE) ? lds4b[lane] : init2;
#pragma unroll
    for (int offset = 2; offset > 0; offset >>= 1) {
      v1 = op1(v1, __shfl_down(v1, offset, WAVE_SIZE));
      v2 = op2(v2, __shfl_down(v2, offset, WAVE_SIZE));
    }
  }
}

// Tile partials at or below which phase C reduces them itself (N <= 2048:
// at most 4 loads per candidate per thread). Above it the redundant read
// grows with N^2 and phase B2 with its barrier stays.
#define FOLD_MAX_TILES 1024

// Reduces the tile partials of ALL candidates at once, in phase B2's exact
// order: thread tid adds w = tid, tid + 256, ... sequentially, then the
// shuffle tree of block_reduce runs per candidate. Wave v leaves
// candidate q's wave partial in wp[v * VZ_QF_QMAX + q]; after ONE
// __syncthreads, fold_quad(wp, q) is bit for bit what B2 stores. The loads
// of a trip are issued together (rows past the batch re-read its last
// row, so the unrolled loop has no branch that would wait per candidate).
//
// `tid` is the thread's index among the BLOCK threads that reduce: the
// continuous and the mixed kernel reduce on half 0 (reduce_all_partials,
// tid = threadIdx.x); the multi-objective kernel gives each half a metric
// (eagle_sweep_mo.hip, tid = threadIdx.x % BLOCK).
__device__ __forceinline__ void reduce_all_partials_at(
    const float* var_ws, int batch_size, int total_tiles, float* wp,
    const int tid) {
  float sacc[VZ_QF_QMAX];
#pragma unroll
  for (int q = 0; q < VZ_QF_QMAX; ++q) sacc[q] = 0.0f;
  for (int w0 = 0; w0 < total_tiles; w0 += BLOCK) {
    const int w = w0 + tid;
    const bool live = w < total_tiles;
    const int wc = live ? w : total_tiles - 1;
    float v[VZ_QF_QMAX];
#pragma unroll
    for (int q = 0; q < VZ_QF_QMAX; ++q) {
      const int qc = min(q, batch_size - 1);
      v[q] = cload(var_ws + (long)qc * (total_tiles + 1) + wc);
    }
#pragma unroll
    for (int q = 0; q < VZ_QF_QMAX; ++q) {
      sacc[q] = live ? sacc[q] + v[q] : sacc[q];
    }
  }
  // The shuffle tree of block_reduce, for all VZ_QF_QMAX candidates in 32
  // shuffles where one tree each would take 6 x 32. A tree level with
  // offset `off` computes v[p] + v[p + off] for positions p < off and
  // nothing else reaches lane 0, so half the lanes of every level are
  // idle: level `off` packs two registers into one, the lanes with
  // (lane & off) == 0 doing the first register's adds and the others the
  // second's. Each add has the operands of the original tree (swapped in
  // the upper lanes; fp add commutes), so the sums are bit-identical.
  // After the off = 2 level one register holds candidate q at the lanes
  // 2 * bitreverse5(q) + {0, 1}; the last level adds the pair.
  const int lane = tid & (WAVE_SIZE - 1);
#pragma unroll
  for (int off = WAVE_SIZE / 2; off > 1; off >>= 1) {
    const bool up = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < off / 2; ++i) {
      const float keep = up ? sacc[2 * i + 1] : sacc[2 * i];
      const float send = up ? sacc[2 * i] : sacc[2 * i + 1];
      sacc[i] = keep + __shfl_xor(send, off, WAVE_SIZE);
    }
  }
  const float total = sacc[0] + __shfl_xor(sacc[0], 1, WAVE_SIZE);
  if ((lane & 1) == 0) {
    const int q = (int)(__brev((unsigned)(lane >> 1)) >> 27);
    wp[(tid / WAVE_SIZE) * VZ_QF_QMAX + q] = total;
  }
}

__device__ __forceinline__ void reduce_all_partials(
    const float* var_ws, int batch_size, int total_tiles, float* wp) {
  reduce_all_partials_at(var_ws, batch_size, total_tiles, wp, threadIdx.x);
}

// block_reduce's second stage over the 4 wave partials: lanes 0..3 hold
// v0..v3, shuffle offsets 2 then 1 give (v0 + v2) + (v1 + v3).
__device__ __forceinline__ float fold_quad(const float* wp, int q) {
  return (wp[q] + wp[2 * VZ_QF_QMAX + q]) +
         (wp[VZ_QF_QMAX + q] + wp[3 * VZ_QF_QMAX + q]);
}

// The sweep's own form of vz_quadform_tile (common.h): every partial is
// produced by the same operations on the same operands in the same order,
// so the two stay bit-identical; only when the loads are issued differs.
// The shared routine's staging loop exposes one memory-side round trip per
// load (the guarded ternary around the relaxed atomic load keeps the
// compiler from batching them): 16 dependent round trips per tile. Here a
// thread puts its 16 loads of k_i / k_j in flight before the first wait.
// Elements outside the batch or the tile re-read a clamped address and
// are replaced by the zero the shared routine stores; a branch around the
// load would bring the waits back.
//
// Called by all SWEEP_THREADS threads, once per trip of phase B. Each half
// of the workgroup (BLOCK threads: `tid` is the thread's index within its
// half, 0 .. BLOCK - 1, the shared routine's threadIdx.x) works on a tile
// and a staging area of its own, so two tiles are in flight per workgroup
// and two waves share each SIMD, each covering the other's LDS and L2
// waits. `live` is uniform over a half: a half without a tile in this trip
// does no loads and no stores, but takes both __syncthreads, which stand
// outside every condition.
template <typename LoadK, typename StoreP>
__device__ __forceinline__ void vz_quadform_tile_pipelined(
    const float* __restrict__ kinv, int b, int n, int tile, int tiles_n,
    int tid, bool live, float* k_i_lds, float* k_j_lds, LoadK loadk,
    StoreP store, unsigned long long* prof = nullptr) {
  constexpr int kStage = VZ_QF_QMAX * VZ_QF_TILE / BLOCK;  // 8 per thread
  const bool profme = (prof != nullptr && threadIdx.x == 0);
  unsigned long long tq0 = profme ? wall_clock64() : 0;
  const int ti = tile / tiles_n, tj = tile % tiles_n;
  const int i0 = ti * VZ_QF_TILE, j0 = tj * VZ_QF_TILE;
  const int ilen = min(VZ_QF_TILE, n - i0);
  const int jlen = min(VZ_QF_TILE, n - j0);
  if (live) {
    // e = tid + u * BLOCK: the column c is the same for every u.
    const int c = tid % VZ_QF_TILE;
    const int q0 = tid / VZ_QF_TILE;
    const int ci = i0 + min(c, ilen - 1), cj = j0 + min(c, jlen - 1);
    float ri[kStage], rj[kStage];
#pragma unroll
    for (int u = 0; u < kStage; ++u) {
      const long base =
          (long)min(q0 + u * (BLOCK / VZ_QF_TILE), b - 1) * n;
      ri[u] = loadk(base + ci);
      rj[u] = loadk(base + cj);
    }
#pragma unroll
    for (int u = 0; u < kStage; ++u) {
      const bool inq = q0 + u * (BLOCK / VZ_QF_TILE) < b;
      k_i_lds[tid + u * BLOCK] = (inq && c < ilen) ? ri[u] : 0.0f;
      k_j_lds[tid + u * BLOCK] = (inq && c < jlen) ? rj[u] : 0.0f;
    }
  }
  __syncthreads();  // all eight waves, live or not
  if (profme) {
    const unsigned long long tq1 = wall_clock64();
    prof[0] += tq1 - tq0;
    tq0 = tq1;
  }
  if (live) {
    const int wave = tid / WAVE_SIZE;
    const int lane = tid % WAVE_SIZE;
    float acc[8];
#pragma unroll
    for (int qq = 0; qq < 8; ++qq) acc[qq] = 0.0f;
    if (lane < jlen) {
      if (ilen == VZ_QF_TILE) {
        for (int ib = 0; ib < VZ_QF_TILE; ib += 8) {
          float kvv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            kvv[u] = kinv[(long)(i0 + ib + u) * n + j0 + lane];
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) {
#pragma unroll
            for (int qq = 0; qq < 8; ++qq) {
              acc[qq] = fmaf(
                  k_i_lds[(wave * 8 + qq) * VZ_QF_TILE + ib + u],
                  kvv[u], acc[qq]);
            }
          }
        }
      } else {
        for (int i = 0; i < ilen; ++i) {
          const float kv = kinv[(long)(i0 + i) * n + j0 + lane];
#pragma unroll
          for (int qq = 0; qq < 8; ++qq) {
            acc[qq] = fmaf(k_i_lds[(wave * 8 + qq) * VZ_QF_TILE + i], kv,
                           acc[qq]);
          }
        }
      }
    }
#pragma unroll
    for (int qq = 0; qq < 8; ++qq) {
      const int q = wave * 8 + qq;
      float v = acc[qq] * k_j_lds[q * VZ_QF_TILE + lane];
      v = wave_reduce_sum(v);
      if (lane == 0 && q < b) store(q, v);
    }
  }
  __syncthreads();  // all eight waves, live or not
  if (profme) prof[1] += wall_clock64() - tq0;
}

// matern52_of_d2 (common.h) with the roundings it has in the rolled
// k-vector loop of the step path: 1 + sr is rounded, then one fma adds
// sr^2 / 3. Inlined into the unrolled four-row loop below, the shared
// function also gets 1 + sqrt(5) r fused into an fma, which changes the
// last bit of the k-vector; spelled out here so that it cannot.
__device__ __forceinline__ float sweep_matern52(float d2) {
#pragma clang fp contract(off)
  const float r = sqrtf(fmaxf(d2, 0.0f));
  const float sr = 2.2360679774997896f * r;  // sqrt(5) * r
  const float one_sr = 1.0f + sr;
  return fmaf(sr * sr, 1.0f / 3.0f, one_sr) * __expf(-sr);
}

// The k-vector loop of phase A (sweep_kvec, sweep_kvec_mixed) keeps the
// loads of up to KV_ROWS rows and KV_CHUNK dimensions in flight together.
#define KV_ROWS 4
#define KV_CHUNK 4
// Phase A's suggest step: dimensions per chunk of the squared distance,
// fireflies per chunk of the weighted sum.
#define SG_DCHUNK 8
#define SG_PCHUNK 16
