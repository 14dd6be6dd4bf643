// Persistent cooperative Eagle-sweep megakernel for gfx950 (v2).
//
// Runs the ENTIRE steady-state acquisition sweep (suggest -> GP
// posterior score -> update, x thousands of iterations) inside ONE
// cooperatively-launched kernel. The hipGraph path replays ~5 kernels
// per iteration at ~85 us/iteration — dispatch-bound, not work-bound.
//
// MI355X coherence design (the crux): the 8 per-XCD L2s are NOT
// cross-coherent, and generic device-scope fences (cg::grid.sync /
// __threadfence) writeback+invalidate L2 — measured ~65 us per sync,
// which made a v1 of this kernel SLOWER than the graph path. v2
// instead:
//   - routes ONLY the small inter-phase buffers (pool state, k-vector,
//     quadform partials, mu/dist) through agent-scope RELAXED atomic
//     loads/stores — coherent at the memory side, no cache flush;
//   - keeps the heavy read-only data (K^-1, x, alpha) on the normal
//     cached path (L2-resident across all iterations);
//   - uses a hand-rolled grid barrier on ONE agent-scope counter that
//     only grows (grid_sync below; s_waitcnt 0 before arrival orders the
//     relaxed data stores);
//   - merges phases so a single workgroup owns candidate b through
//     suggest+k-vec (A); only the quadform (B) fans out across the grid.
//
// Phases and grid barriers per iteration. Two grid-uniform switches pick
// among four forms:
//   resident  pool_size * dc <= RESIDENT_CAP (4096 floats)
//   folded    tile partials T <= FOLD_MAX_TILES (1024, i.e. N <= 2048)
//
//   resident, folded  (flagship)   A | B | RC                 2 barriers
//   resident, not folded           A | B | B2 | RC            3 barriers
//   legacy, folded                 A | B | C |                3 barriers
//   legacy, not folded             A | B | B2 | C |           4 barriers
//
// Folded: B2 and its barrier existed to hand 25 floats over. Every
// workgroup that runs C / RC needs all scores anyway, so it reduces the
// partials of all candidates itself, in B2's exact order
// (reduce_all_partials), and the owner of candidate q still stores the
// reduced value to var_ws[q, T] for the caller.
//
// Resident: every workgroup that owns a candidate (blockIdx.x <
// batch_size) loads pool, rewards, perturbations and best_reward once at
// kernel start into LDS (the upper half of pool_lds, which phase B's
// k_i / k_j staging does not touch: half 0 stages in the lower half and
// half 1 in stage1_lds; plus st_rewards / st_perts / st_best)
// and keeps them for the whole launch. RC = reduce + scores + update:
// each owner applies the update of ALL batch_size fireflies, with the
// logic and RNG indices of the legacy phase C, to its own copy. The
// inputs (all scores, all candidates, the old state) are the same for
// every owner, so the copies stay identical, nobody reads another's
// state, and the next A follows RC with no grid barrier and no restaging
// of the pool. After the last iteration workgroup 0 stores its copy back.
// Workgroups that own no candidate skip A and RC. With a grid below the
// batch, A loops over its candidates and RC runs once per workgroup.
//
// Parity scratch (resident mode). With no barrier after RC, a fast
// workgroup's A(it+1) would overwrite candidate, mu and dist of its row
// while a slow one still reads them in RC(it). So A(it) also writes them
// to slot it & 1 of slot_ws (2 x batch x (dc + 2) floats, allocated by
// the binding, cstore) and RC(it) reads only that slot (cload). This is
// race-free by construction, not by timing: A(it+1) writes the OTHER
// slot; the next writer of slot it & 1 is A(it+2), and a workgroup gets
// there only through barrier A|B of it+1, at which every workgroup has
// arrived only after finishing its RC(it). The caller-visible out_cont,
// mu_ws and dist_ws are still written by A, for the tests; nothing in
// resident mode reads them. k_ws and the tile partials are written and
// read only across the barriers that remain (A|B and B|RC), and
// var_ws[q, T] is written by one owner and read by no one when folded.
//
// Legacy (pool_size * dc > RESIDENT_CAP): the state lives in global
// memory behind cload / cstore, A stages the pool in LDS per iteration up
// to POOL_LDS_CAP floats and reads it through cload above, the owner of
// candidate i updates firefly i in C, and a barrier separates C from the
// next A.
//
// Workgroup shape: 512 threads, eight waves, two per SIMD, on at most 128
// workgroups (the barrier's cost grows with the arrivals on its one word,
// so the second tile of a CU comes from more waves, not more workgroups).
// Phase B gives each half of 256 threads a tile and a staging area of its
// own (half 0 the lower half of pool_lds, half 1 stage1_lds): tile
// blockIdx.x + G * (2 * trip + half). A lone wave issues fp32 fma at half
// the SIMD's rate and nothing covers its LDS and L2 waits; two waves per
// SIMD cover each other's. Which half computes a tile partial does not
// change its operations or their order. Phases A, B2 and C / RC are the
// 256-thread arithmetic of the step kernels on half 0 (same rows per
// thread, same chains, same 4-wave reduction order: sweep_block_reduce);
// the `+= BLOCK` loops of a half-1 thread start at SWEEP_IDLE and make no
// trip, and tests like tid == 0 are false for it.
//
// Every __syncthreads must be reached by all eight waves, so none stands
// under a condition that differs within a workgroup. The sites, and why:
//   grid_sync (two each)       called at the top level of the iteration
//                              loop, under the grid-uniform `fold` and
//                              `resident` only
//   sweep_block_reduce[2]      called from the sites below, unconditionally
//   prologue state load        under resident && owner: owner is
//                              blockIdx.x < batch_size
//   phase A                    all inside the loop over b = blockIdx.x +
//                              k G, straight-line except `stage_pool`
//                              (grid-uniform)
//   vz_quadform_tile_pipelined two, outside `if (live)`; the trip loop
//                              runs on tile0 = blockIdx.x + 2 G trip, the
//                              same for both halves
//   phase B2                   loop over q = blockIdx.x + k G
//   RC                         under resident && owner; `half == 0` guards
//                              only reduce_all_partials, which has none
//   legacy C                   under fold && owner, then the loop over
//                              i = blockIdx.x + k G
// Conditions on `half`, `live`, `tid` or `lane` enclose loads, stores and
// arithmetic only.
//
// Scope: continuous-only spaces, q == 1 (the flagship GP-Bandit
// config); the optimizer falls back to the hipGraph path otherwise.
//
// Determinism: phases replicate the standalone kernels VERBATIM (same
// counter-based RNG streams, same 64x64 tile quadform and partial
// order, same block-reduce orders; where a loop is restructured to keep
// its loads in flight, vz_quadform_tile_pipelined, sweep_kvec and the
// chunked loops of phase A's suggest step below, or two reductions share
// one barrier pass (sweep_block_reduce2),
// every value still comes from the same operations on the same operands
// in the same order), so for N < 4096 the sweep is
// BIT-IDENTICAL to the step kernels of the hipGraph path for the same
// seeds: the whole pool state, asserted by tests/test_sweep_kernel.py
// and tests/test_gpu_ops.py. For 4096 <= N <= 8192 the standalone
// scorer switches to a row-split k-vector kernel plus one SGEMM
// (module.cpp, gemm_n_threshold) while the sweep keeps this file's
// k-vector loop and the tiles, so the two paths sum in different orders
// and agree only to the fp64-oracle tolerance; that range is held to
// the fp64 oracle phase by phase (tests/test_sweep_kernel.py).
//
// Deadlock safety: every phase is a grid-stride loop (any grid size is
// correct: grids of 1, 7 and 200 workgroups are run by
// tests/test_sweep_kernel.py); the launcher clamps the grid to the
// cooperative occupancy limit, and cooperative launch guarantees
// co-residency.

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
__device__ __forceinline__ void reduce_all_partials(
    const float* var_ws, int batch_size, int total_tiles, float* wp) {
  const int tid = threadIdx.x;
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

// Phase A's k-vector, mu and trust-region distance of one candidate: the
// loop of the step path (row = tid, tid + BLOCK, ...; j = 0 .. dc - 1 per
// row; mu_acc and min_linf over the thread's rows in that order), with the
// loads of up to KV_ROWS rows and KV_CHUNK dimensions in flight together.
// The rolled form did one load of x, one of xq and one of inv_ls per
// dimension and waited for all three: rows x dc serialized round trips
// per thread; this one exposes dc / KV_CHUNK per KV_ROWS rows. (Loading
// the next chunk while this one is used did not survive the compiler,
// which moves the load back to the head of the trip.) VEC4 reads x
// as float4 (dc a multiple of 4, x 16-byte aligned; chosen once per
// launch); otherwise each element is loaded on its own. Rows past n and
// dimensions past dc re-read a clamped address and are discarded.
#define KV_ROWS 4
#define KV_CHUNK 4
// Phase A's suggest step: dimensions per chunk of the squared distance,
// fireflies per chunk of the weighted sum.
#define SG_DCHUNK 8
#define SG_PCHUNK 16

template <bool VEC4>
__device__ __forceinline__ void sweep_kvec(
    const float* __restrict__ x, const float* __restrict__ inv_ls,
    const float* __restrict__ alpha, const float* xq_lds, float* k_row,
    int dc, int n, int wt, float amp2, float& mu_acc, float& min_linf) {
  for (int row0 = wt; row0 < n; row0 += KV_ROWS * BLOCK) {
    const float* xr[KV_ROWS];
    float al[KV_ROWS];
#pragma unroll
    for (int s = 0; s < KV_ROWS; ++s) {
      const int rc = min(row0 + s * BLOCK, n - 1);
      xr[s] = x + (long)rc * dc;
      al[s] = alpha[rc];
    }
    auto load_chunk = [&](float (&buf)[KV_ROWS][KV_CHUNK], int j0) {
#pragma unroll
      for (int s = 0; s < KV_ROWS; ++s) {
        if (VEC4) {
          const float4 v = *reinterpret_cast<const float4*>(xr[s] + j0);
          buf[s][0] = v.x; buf[s][1] = v.y; buf[s][2] = v.z; buf[s][3] = v.w;
        } else {
#pragma unroll
          for (int c = 0; c < KV_CHUNK; ++c) {
            buf[s][c] = xr[s][min(j0 + c, dc - 1)];
          }
        }
      }
    };
    float d2[KV_ROWS], linf[KV_ROWS];
#pragma unroll
    for (int s = 0; s < KV_ROWS; ++s) d2[s] = linf[s] = 0.0f;
    for (int j0 = 0; j0 < dc; j0 += KV_CHUNK) {
      float cur[KV_ROWS][KV_CHUNK];
      load_chunk(cur, j0);
      float xq[KV_CHUNK], il[KV_CHUNK];
#pragma unroll
      for (int c = 0; c < KV_CHUNK; ++c) {
        const int jc = VEC4 ? j0 + c : min(j0 + c, dc - 1);
        xq[c] = xq_lds[jc];
        il[c] = inv_ls[jc];
      }
#pragma unroll
      for (int c = 0; c < KV_CHUNK; ++c) {
        if (VEC4 || j0 + c < dc) {
#pragma unroll
          for (int s = 0; s < KV_ROWS; ++s) {
            const float diff = xq[c] - cur[s][c];
            const float z = diff * il[c];
            d2[s] = fmaf(z, z, d2[s]);
            linf[s] = fmaxf(linf[s], fabsf(diff));  // continuous-only
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < KV_ROWS; ++s) {
      const int row = row0 + s * BLOCK;
      const bool live = row < n;
      const float kv = amp2 * sweep_matern52(d2[s]);
      if (live) cstore(k_row + row, kv);
      mu_acc = live ? fmaf(kv, al[s], mu_acc) : mu_acc;
      min_linf = live ? fminf(min_linf, linf[s]) : min_linf;
    }
  }
}

extern "C" __global__ __launch_bounds__(SWEEP_THREADS) void
eagle_sweep_kernel(
    float* __restrict__ pool_cont,         // (P, Dc)   [coherent]
    float* __restrict__ rewards,           // (P,)      [coherent]
    float* __restrict__ perturbations,     // (P,)      [coherent]
    float* __restrict__ best_reward,       // (1,)      [coherent]
    unsigned long long* __restrict__ iter_ptr,  // (2,)
    unsigned int* __restrict__ barrier_buf,     // (2,) zeroed
    const float* __restrict__ x,           // (N, D)    [cached]
    const float* __restrict__ inv_ls,      // (D,)      [cached]
    const float* __restrict__ alpha,       // (N,)      [cached]
    const float* __restrict__ kinv,        // (N, N)    [cached]
    float* __restrict__ out_cont,          // (B, Dc)   [wg-private]
    float* __restrict__ k_ws,              // (B, N)    [coherent]
    float* __restrict__ mu_ws,             // (B,)      [coherent]
    float* __restrict__ dist_ws,           // (B,)      [coherent]
    float* __restrict__ var_ws,            // (B, T+1)  [coherent]
    float* __restrict__ slot_ws,           // (2, B*(Dc+2)) [coherent]
    int n_batches, int batch_size, int pool_size, int dc, int n,
    long long it_start, long long iterations,
    float visibility, float gravity, float neg_gravity, float norm_scale,
    float penalize_factor, float perturbation_lower_bound,
    float base_perturbation,
    unsigned long long seed_suggest, unsigned long long seed_update,
    float amp2, float mean_c, int acq, float coef, float best_value,
    float tr_radius) {
  __shared__ float scale[MAX_POOL];
  __shared__ float red[8];
  __shared__ float red2[4];  // second value of sweep_block_reduce2
  __shared__ float s_scalar;
  __shared__ __attribute__((aligned(16))) float xq_lds[512];
  __shared__ float pool_lds[POOL_LDS_CAP];
  // Phase B's k_i / k_j staging of half 1 (half 0 stages in pool_lds).
  __shared__ float stage1_lds[2 * VZ_QF_QMAX * VZ_QF_TILE];
  // Resident mode: this workgroup's private copy of the Eagle state.
  __shared__ float st_rewards[MAX_POOL];
  __shared__ float st_perts[MAX_POOL];
  __shared__ float st_best;

  const int tid = threadIdx.x;
  // Half of the workgroup (wave-uniform) and the thread's index in it.
  const int half = tid / BLOCK;
  const int htid = tid % BLOCK;
  // Start of every `+= BLOCK` loop of the BLOCK-thread phases: half 1
  // makes no trip. Tests like tid == 0 and tid < batch_size are false for
  // half 1 as they stand.
  const int wt = half == 0 ? tid : SWEEP_IDLE;
  const int G = gridDim.x;
  const int pool_elems = pool_size * dc;
  // All three are grid-uniform: every workgroup takes the same barriers.
  const bool resident = pool_elems <= RESIDENT_CAP;
  const bool stage_pool = !resident && pool_elems <= POOL_LDS_CAP;
  const bool pool_in_lds = resident || stage_pool;
  const bool owner = blockIdx.x < batch_size;
  // Form of the k-vector loop (sweep_kvec), picked once per launch.
  const bool x_vec4 = dc % KV_CHUNK == 0 &&
                      (reinterpret_cast<unsigned long long>(x) & 15) == 0;
  float* st_pool = pool_lds + RESIDENT_CAP;
  const float* pl = resident ? st_pool : pool_lds;
  auto fsum = [](float a, float c) { return a + c; };
  auto fmin_ = [](float a, float c) { return fminf(a, c); };
  auto fmax_ = [](float a, float c) { return fmaxf(a, c); };

  // Per-phase cycle profiling (workgroup 0's view, including its
  // barrier-wait slack): accumulated into iter_ptr[2..9] as
  // A, barA, B, barB, B2, barB2, RC (legacy: C), barC. A phase or
  // barrier the mode does not take leaves its slot untouched: B2 / barB2
  // when folded, barC when resident. Reads are a handful of s_memtime
  // per iteration on one lane — no measurable perturbation.
  const bool profwg = (blockIdx.x == 0 && threadIdx.x == 0);
  unsigned long long tmark = profwg ? wall_clock64() : 0;
  unsigned int bar_target = 0;  // (barriers passed) * G, see grid_sync
#define VZ_SWEEP_PROF(slot)                                        \
  if (profwg) {                                                    \
    const unsigned long long tnow = wall_clock64();                \
    iter_ptr[2 + (slot)] += tnow - tmark;                          \
    tmark = tnow;                                                  \
  }

  // Resident mode: the state was written by earlier launches, so plain
  // loads see it; from here on only this workgroup touches its copy.
  if (resident && owner) {
    for (int e = wt; e < pool_elems; e += BLOCK) st_pool[e] = pool_cont[e];
    for (int p = wt; p < pool_size; p += BLOCK) {
      st_rewards[p] = rewards[p];
      st_perts[p] = perturbations[p];
    }
    if (tid == 0) st_best = best_reward[0];
    __syncthreads();
  }

  for (long long it = it_start; it < it_start + iterations; ++it) {
    const unsigned long long offset = (unsigned long long)it;
    // Parity slot of this iteration: candidates, then mu, then dist.
    float* slot_c = slot_ws + (long)(it & 1) * batch_size * (dc + 2);
    float* slot_mu = slot_c + batch_size * dc;
    float* slot_dist = slot_mu + batch_size;
    const int batch_start =
        (int)(offset % (unsigned long long)n_batches) * batch_size;
    if (profwg) tmark = wall_clock64();

    // ---- Phase A: suggest + k-vec (workgroup owns candidate b) ----
    for (int b = blockIdx.x; b < batch_size; b += G) {
      if (stage_pool) {
        for (int e = wt; e < pool_elems; e += BLOCK) {
          pool_lds[e] = cload(pool_cont + e);
        }
        __syncthreads();
      }
      const int me = batch_start + b;
      const float my_reward = resident ? st_rewards[me]
                                       : cload(rewards + me);
      const float my_pert = resident ? st_perts[me]
                                     : cload(perturbations + me);
      // Squared distance over SG_DCHUNK dimensions at a time: the loads
      // of a chunk (LDS, or memory-side when the pool is not staged) are
      // issued together, then the chain runs j = 0 .. dc - 1 as in the
      // step kernel. Dimensions past dc re-read dc - 1 and are dropped.
      auto dist2 = [&](auto ld, int p) {
        float d2 = 0.0f;
        for (int j0 = 0; j0 < dc; j0 += SG_DCHUNK) {
          float mv[SG_DCHUNK], pv[SG_DCHUNK];
#pragma unroll
          for (int u = 0; u < SG_DCHUNK; ++u) {
            const int jc = min(j0 + u, dc - 1);
            mv[u] = ld(me * dc + jc);
            pv[u] = ld(p * dc + jc);
          }
#pragma unroll
          for (int u = 0; u < SG_DCHUNK; ++u) {
            const float diff = mv[u] - pv[u];
            d2 = (j0 + u < dc) ? fmaf(diff, diff, d2) : d2;
          }
        }
        return d2;
      };
      auto ld_lds = [&](int idx) { return pl[idx]; };
      auto ld_mem = [&](int idx) { return cload(pool_cont + idx); };
      for (int p = wt; p < pool_size; p += BLOCK) {
        const float d2 = pool_in_lds ? dist2(ld_lds, p) : dist2(ld_mem, p);
        const float reward_p = resident ? st_rewards[p]
                                        : cload(rewards + p);
        const float dir = (reward_p - my_reward >= 0.0f) ? gravity
                                                         : -neg_gravity;
        const float force = __expf(-visibility * d2 / dc * 10.0f);
        float s = dir * force;
        if (!isfinite(reward_p)) s = 0.0f;
        scale[p] = s;
      }
      __syncthreads();
      float pulls = 0.0f, pushes = 0.0f;
      for (int p = wt; p < pool_size; p += BLOCK) {
        pulls += (scale[p] > 0.0f) ? 1.0f : 0.0f;
        pushes += (scale[p] < 0.0f) ? 1.0f : 0.0f;
      }
      // Both counts on one barrier pass (red / red2), each in
      // block_reduce's order.
      sweep_block_reduce2(pulls, pushes, red, red2, fsum, fsum, 0.0f, 0.0f);
      if (tid == 0) {
        red[4] = fmaxf(pulls, 1.0f);
        red[5] = fmaxf(pushes, 1.0f);
      }
      __syncthreads();
      const float inv_pull = 1.0f / red[4];
      const float inv_push = 1.0f / red[5];
      float ssum = 0.0f;
      for (int p = wt; p < pool_size; p += BLOCK) {
        const float s = scale[p];
        const float ns = norm_scale * (s > 0.0f ? s * inv_pull
                                                : s * inv_push);
        scale[p] = ns;
        ssum += ns;
      }
      __syncthreads();
      float scale_sum = sweep_block_reduce(ssum, red, fsum, 0.0f);
      if (tid == 0) s_scalar = scale_sum;
      __syncthreads();
      scale_sum = s_scalar;
      // The weighted sum over SG_PCHUNK fireflies at a time, chain in
      // the order p = 0 .. pool_size - 1; fireflies past the pool re-read
      // the last one and are dropped.
      auto moved_of = [&](auto ld, int j) {
        float moved = 0.0f;
        for (int p0 = 0; p0 < pool_size; p0 += SG_PCHUNK) {
          float sv[SG_PCHUNK], pv[SG_PCHUNK];
#pragma unroll
          for (int u = 0; u < SG_PCHUNK; ++u) {
            const int pc = min(p0 + u, pool_size - 1);
            sv[u] = scale[pc];
            pv[u] = ld(pc * dc + j);
          }
#pragma unroll
          for (int u = 0; u < SG_PCHUNK; ++u) {
            moved = (p0 + u < pool_size) ? fmaf(sv[u], pv[u], moved)
                                         : moved;
          }
        }
        return moved;
      };
      for (int j = wt; j < dc; j += BLOCK) {
        float moved = pool_in_lds ? moved_of(ld_lds, j)
                                  : moved_of(ld_mem, j);
        const float mine = pool_in_lds ? pl[me * dc + j]
                                       : cload(pool_cont + me * dc + j);
        moved = mine + (moved - mine * scale_sum);
        float noise = vz_rng_laplace<float>(seed_suggest, offset,
                                     (unsigned)(b * dc + j));
        noise = (noise >= 0.0f) ? 1.0f : -1.0f;  // q == 1
        const float cand = moved + noise * my_pert;
        out_cont[b * dc + j] = cand;
        if (resident) cstore(slot_c + b * dc + j, cand);
        xq_lds[j] = cand;
      }
      __syncthreads();

      // k-vector + mu + trust-region distance for candidate b.
      float mu_acc = 0.0f;
      float min_linf = INFINITY;
      if (x_vec4) {
        sweep_kvec<true>(x, inv_ls, alpha, xq_lds, k_ws + (long)b * n, dc,
                         n, wt, amp2, mu_acc, min_linf);
      } else {
        sweep_kvec<false>(x, inv_ls, alpha, xq_lds, k_ws + (long)b * n, dc,
                          n, wt, amp2, mu_acc, min_linf);
      }
      // mu and dist on one barrier pass, as the two counts above.
      sweep_block_reduce2(mu_acc, min_linf, red, red2, fsum, fmin_, 0.0f,
                          INFINITY);
      if (tid == 0) {
        cstore(mu_ws + b, mu_acc);
        cstore(dist_ws + b, min_linf);
        if (resident) {
          cstore(slot_mu + b, mu_acc);
          cstore(slot_dist + b, min_linf);
        }
      }
      __syncthreads();
    }
    VZ_SWEEP_PROF(0)
    grid_sync(barrier_buf, bar_target);
    VZ_SWEEP_PROF(1)

    // ---- Phase B: K^-1 quadform (64x64 tiles, Kinv read ONCE) ----
    // Shared template with the standalone chunked scorer
    // (vz_quadform_tile in common.h): identical float-op order keeps
    // the megakernel bit-identical to the hipGraph path wherever that
    // path takes the tile quadform too (N < 4096). var_ws layout is
    // (B, T+1): T tile partials + the reduced quadform.
    {
      const int tiles_n = (n + VZ_QF_TILE - 1) / VZ_QF_TILE;
      const int total_tiles = tiles_n * tiles_n;
      // Half h stages k_i / k_j (2048 floats each) in an area of its own
      // and takes tile blockIdx.x + G * (2 * trip + h): the tiles of a
      // trip go to the half-0s of all workgroups first, so the halves of
      // one workgroup are two waves per SIMD only once every CU of the
      // grid has a tile. The trip count is the same for every wave of the
      // grid-stride loop; a half past the last tile runs the trip with
      // live == false (the routine's barriers are unconditional).
      float* k_i_lds = half == 0 ? pool_lds : stage1_lds;
      float* k_j_lds = k_i_lds + VZ_QF_QMAX * VZ_QF_TILE;
      for (int tile0 = blockIdx.x; tile0 < total_tiles; tile0 += 2 * G) {
        const int t = tile0 + half * G;
        vz_quadform_tile_pipelined(
            kinv, batch_size, n, t, tiles_n, htid, t < total_tiles,
            k_i_lds, k_j_lds,
            [&](long idx) { return cload(k_ws + idx); },
            [&](int q, float v) {
              cstore(var_ws + (long)q * (total_tiles + 1) + t, v);
            },
            blockIdx.x == 0 ? iter_ptr + 10 : nullptr);
      }
    }
    VZ_SWEEP_PROF(2)
    grid_sync(barrier_buf, bar_target);
    VZ_SWEEP_PROF(3)

    // ---- Phase B2: reduce tile partials (order == the standalone
    // ps_reduce_parts_kernel). Only above FOLD_MAX_TILES; below it
    // phase C reduces them itself and this barrier is not taken. ----
    const int tiles_n_c = (n + VZ_QF_TILE - 1) / VZ_QF_TILE;
    const int total_tiles_c = tiles_n_c * tiles_n_c;
    const bool fold = total_tiles_c <= FOLD_MAX_TILES;  // grid-uniform
    if (!fold) {
      for (int q = blockIdx.x; q < batch_size; q += G) {
        float sacc = 0.0f;
        for (int w = wt; w < total_tiles_c; w += BLOCK) {
          sacc += cload(var_ws + (long)q * (total_tiles_c + 1) + w);
        }
        float total = sweep_block_reduce(sacc, red, fsum, 0.0f);
        if (tid == 0) {
          cstore(var_ws + (long)q * (total_tiles_c + 1) + total_tiles_c,
                 total);
        }
        __syncthreads();
      }
      VZ_SWEEP_PROF(4)
      grid_sync(barrier_buf, bar_target);
      VZ_SWEEP_PROF(5)
    }

    // ---- Phase C / RC: reduce (when folded) + scores + update ----
    // Scratch in phase B's staging area, free until the next phase B:
    // 4 x VZ_QF_QMAX wave partials, then VZ_QF_QMAX scores.
    float* wp = pool_lds;
    float* sc_lds = pool_lds + 4 * VZ_QF_QMAX;
    auto score_of = [&](float quad, float mu_raw, float dist) {
      float var = fmaxf(amp2 - quad, 1e-12f);
      const float sd = sqrtf(var);
      const float mu = mu_raw + mean_c;
      return vz_trust_region(vz_acq_score(acq, mu, sd, coef, best_value),
                             dist, tr_radius);
    };
    if (resident) {
      // RC: every owning workgroup applies the update of ALL fireflies
      // of the batch to its own LDS copy of the state, with the logic and
      // RNG indices of the legacy phase C below, and goes straight on to
      // the next phase A: no grid barrier.
      if (owner) {
        float mu_t = 0.0f, dist_t = 0.0f;
        if (tid < batch_size) {
          mu_t = cload(slot_mu + tid);
          dist_t = cload(slot_dist + tid);
        }
        if (fold && half == 0) {
          reduce_all_partials(var_ws, batch_size, total_tiles_c, wp);
        }
        __syncthreads();
        if (tid < WAVE_SIZE) {  // batch <= VZ_QF_QMAX < WAVE_SIZE
          float score = -INFINITY;
          if (tid < batch_size) {
            float* reduced =
                var_ws + (long)tid * (total_tiles_c + 1) + total_tiles_c;
            float quad;
            if (fold) {
              quad = fold_quad(wp, tid);
              // The owner of candidate tid publishes the reduced value.
              if (tid % G == (int)blockIdx.x) cstore(reduced, quad);
            } else {
              quad = cload(reduced);
            }
            score = score_of(quad, mu_t, dist_t);
            sc_lds[tid] = score;
          }
          // block_reduce's max over the batch: waves 1..3 would only
          // contribute -inf.
          const float batch_max = wave_reduce_max(score);
          if (tid == 0) s_scalar = fmaxf(st_best, batch_max);
        }
        __syncthreads();
        const float new_best = s_scalar;
        for (int e = wt; e < batch_size * dc; e += BLOCK) {
          const int i = e / dc;
          const int me = batch_start + i;
          const int ej = me * dc + (e - i * dc);
          const float new_r = sc_lds[i];
          const float old_r = st_rewards[me];
          const bool improved = new_r > old_r;
          const float old_pert = st_perts[me];
          const float pert = improved ? old_pert
                                      : old_pert * penalize_factor;
          const float reward = improved ? new_r : old_r;
          const bool dead = (pert < perturbation_lower_bound) &&
                            (reward != new_best);
          if (dead) {
            st_pool[ej] = vz_rng_uniform<float>(
                seed_update, offset ^ 0x5151ull, (unsigned)ej);
          } else if (improved) {
            st_pool[ej] = cload(slot_c + e);
          }
        }
        __syncthreads();  // every read of the old rewards / perts is done
        if (tid < batch_size) {
          const int me = batch_start + tid;
          const float new_r = sc_lds[tid];
          const float old_r = st_rewards[me];
          const bool improved = new_r > old_r;
          const float old_pert = st_perts[me];
          float pert = improved ? old_pert : old_pert * penalize_factor;
          float reward = improved ? new_r : old_r;
          const bool dead = (pert < perturbation_lower_bound) &&
                            (reward != new_best);
          if (dead) {
            reward = -INFINITY;
            pert = base_perturbation;
          }
          st_rewards[me] = reward;
          st_perts[me] = pert;
        }
        if (tid == 0) st_best = new_best;
        __syncthreads();
      }
      VZ_SWEEP_PROF(6)
    } else {
      // Legacy: the state lives in global memory, the owner of candidate
      // i updates firefly i, and a grid barrier separates C from the
      // next A. Folded: an owning workgroup reduces the partials of all
      // candidates once.
      if (fold && owner) {
        if (half == 0) {
          reduce_all_partials(var_ws, batch_size, total_tiles_c, wp);
        }
        __syncthreads();
      }
      for (int i = blockIdx.x; i < batch_size; i += G) {
        // Every workgroup recomputes all B scores from the coherent
        // partials (cheap, deterministic, removes a barrier).
        float local_max = -INFINITY;
        float my_score = -INFINITY;
        for (int t = wt; t < batch_size; t += BLOCK) {
          float* reduced =
              var_ws + (long)t * (total_tiles_c + 1) + total_tiles_c;
          float quad;
          if (fold) {
            quad = fold_quad(wp, t);
            // The owner of candidate t publishes the reduced value.
            if (t == i) cstore(reduced, quad);
          } else {
            quad = cload(reduced);
          }
          const float score =
              score_of(quad, cload(mu_ws + t), cload(dist_ws + t));
          local_max = fmaxf(local_max, score);
          if (t == i) my_score = score;
        }
        float batch_max = sweep_block_reduce(local_max, red, fmax_, -INFINITY);
        // my_score lives in the thread with tid == i%BLOCK (B <= BLOCK):
        // broadcast through LDS.
        if (tid == (i % BLOCK) && i < BLOCK) red[6] = my_score;
        __syncthreads();
        const float new_r = red[6];
        if (tid == 0) {
          s_scalar = fmaxf(cload(best_reward), batch_max);
          if (i == 0) cstore(best_reward, s_scalar);
        }
        __syncthreads();
        const float new_best = s_scalar;
        const int me = batch_start + i;
        const float old_r = cload(rewards + me);
        const bool improved = new_r > old_r;
        const float old_pert = cload(perturbations + me);
        float pert = improved ? old_pert : old_pert * penalize_factor;
        float reward = improved ? new_r : old_r;
        const bool dead = (pert < perturbation_lower_bound) &&
                          (reward != new_best);
        if (improved) {
          for (int j = wt; j < dc; j += BLOCK) {
            cstore(pool_cont + me * dc + j, out_cont[i * dc + j]);
          }
        }
        if (dead) {
          for (int j = wt; j < dc; j += BLOCK) {
            cstore(pool_cont + me * dc + j,
                   vz_rng_uniform<float>(seed_update, offset ^ 0x5151ull,
                                  (unsigned)(me * dc + j)));
          }
          reward = -INFINITY;
          pert = base_perturbation;
        }
        if (tid == 0) {
          cstore(rewards + me, reward);
          cstore(perturbations + me, pert);
        }
        __syncthreads();
      }
      VZ_SWEEP_PROF(6)
      grid_sync(barrier_buf, bar_target);
      VZ_SWEEP_PROF(7)
    }
  }

  // Resident mode: every owner holds the same final state; workgroup 0
  // hands it back. With iterations == 0 nothing changed (and no barrier
  // orders this store after the other workgroups' prologue loads).
  if (resident && blockIdx.x == 0 && iterations > 0) {
    for (int e = wt; e < pool_elems; e += BLOCK) {
      cstore(pool_cont + e, st_pool[e]);
    }
    for (int p = wt; p < pool_size; p += BLOCK) {
      cstore(rewards + p, st_rewards[p]);
      cstore(perturbations + p, st_perts[p]);
    }
    if (tid == 0) cstore(best_reward, st_best);
  }

  if (blockIdx.x == 0 && tid == 0) {
    iter_ptr[0] = (unsigned long long)(it_start + iterations);
    iter_ptr[1] = (unsigned long long)(it_start + iterations - 1);
  }
}

// Host launcher: cooperative launch with occupancy-clamped grid.
// Returns the grid size used, 0 if cooperative launch is unavailable,
// or a negative hipError_t on failure.
extern "C" int launch_eagle_sweep(
    float* pool_cont, float* rewards, float* perturbations,
    float* best_reward, unsigned long long* iter_ptr,
    unsigned int* barrier_buf, const float* x, const float* inv_ls,
    const float* alpha, const float* kinv, float* out_cont, float* k_ws,
    float* mu_ws, float* dist_ws, float* var_ws, float* slot_ws,
    int n_batches,
    int batch_size, int pool_size, int dc, int n, long long it_start,
    long long iterations, float visibility, float gravity,
    float neg_gravity, float norm_scale, float penalize_factor,
    float perturbation_lower_bound, float base_perturbation,
    unsigned long long seed_suggest, unsigned long long seed_update,
    float amp2, float mean_c, int acq, float coef, float best_value,
    float tr_radius, hipStream_t stream) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  int coop = 0;
  (void)hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch,
                              dev);
  if (!coop) return 0;
  int num_cu = 0;
  (void)hipDeviceGetAttribute(&num_cu,
                              hipDeviceAttributeMultiprocessorCount, dev);
  int blocks_per_cu = 0;
  hipError_t err = hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &blocks_per_cu, (const void*)eagle_sweep_kernel, SWEEP_THREADS, 0);
  if (err != hipSuccess || blocks_per_cu < 1) return 0;
  const int tiles_n = (n + VZ_QF_TILE - 1) / VZ_QF_TILE;
  // Grid size is a pure throughput knob (every phase is a grid-stride
  // loop and partial-sum layout is grid-independent, so results are
  // bit-identical at any size). The default is capped at 128 and
  // floored at 64. The cap dates from the sense-reversing barrier,
  // whose cost grew with the arrival count (headline shape, N=1000,
  // batch 25: 256 WGs ran at 61 us/iter, 64-128 WGs at ~42). The
  // barrier on one growing counter (grid_sync) no longer has that cost:
  // the grid tables in profiles/bench_sweep_two_barriers.md and
  // profiles/bench_sweep_loads_in_flight.md. Raising the cap is left to
  // a change of its own, A/B'd over the other shapes;
  // tests/test_sweep_kernel.py asserts 128. The grid counts workgroups
  // of SWEEP_THREADS = 512 threads: each runs two tiles of phase B at
  // once, one per half, so 128 workgroups hold the 256 tiles of the
  // headline shape in one trip with 128 arrivals at the barrier
  // (profiles/bench_sweep_two_tiles.md). The occupancy query and the
  // launch both use 512 threads. The floor: tiles_n^2
  // starves phase A at small N (4 WGs at N=125 ran at 107 us/iter).
  // Override with VIZIER_AMD_SWEEP_GRID.
  int grid = tiles_n * tiles_n;                   // fills phase B
  if (grid > 128) grid = 128;
  if (grid < 64) grid = 64;
  static int grid_env = -1;
  if (grid_env < 0) {
    const char* env = getenv("VIZIER_AMD_SWEEP_GRID");
    grid_env = (env != nullptr) ? atoi(env) : 0;
  }
  if (grid_env > 0) grid = grid_env;
  const int max_grid = blocks_per_cu * num_cu;
  if (grid > max_grid) grid = max_grid;
  if (grid < 1) grid = 1;

  void* args[] = {
      &pool_cont, &rewards, &perturbations, &best_reward, &iter_ptr,
      &barrier_buf, &x, &inv_ls, &alpha, &kinv, &out_cont, &k_ws,
      &mu_ws, &dist_ws, &var_ws, &slot_ws, &n_batches, &batch_size, &pool_size,
      &dc, &n, &it_start, &iterations, &visibility, &gravity,
      &neg_gravity, &norm_scale, &penalize_factor,
      &perturbation_lower_bound, &base_perturbation, &seed_suggest,
      &seed_update, &amp2, &mean_c, &acq, &coef, &best_value,
      &tr_radius};
  err = hipLaunchCooperativeKernel((const void*)eagle_sweep_kernel,
                                   dim3(grid), dim3(SWEEP_THREADS), args, 0,
                                   stream);
  if (err != hipSuccess) return -(int)err;
  return grid;
}
