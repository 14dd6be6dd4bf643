// Tile geometry and the streamed 64 x 64 quadform tile shared by the
// multitask scorer (posterior_score_multitask.hip) and the group scorer
// (posterior_score_group.hip).
#pragma once

#include <hip/hip_runtime.h>
#include "common.h"

#define MT_BLOCK 256
#define MT_ROWS 64     // training rows per tile == WAVE_SIZE (lane = row)
#define MT_COLS 64     // feature columns per LDS chunk
#define MT_LD 65       // row stride of the transposed x tile
#define MT_Q 32        // candidates per group
#define MT_WAVES (MT_BLOCK / WAVE_SIZE)
#define MT_QW (MT_Q / MT_WAVES)  // candidates per wave
#define MT_HALF 32     // rows of a W tile per register buffer
#define MT_KLD 36      // candidate stride of the [row][candidate] k_i slab:
                       // a multiple of 4 (128-bit reads) that spreads the
                       // transposing writes over 8 banks instead of 1
#define MT_GRID_MAX 1024  // quadform grid cap (4 workgroups per CU)

static_assert(MT_ROWS == WAVE_SIZE, "lane = row");
static_assert(MT_QW == 8, "two float4 reads per wave");

#define MT_NOPK __attribute__((target("no-packed-fp32-ops")))

// 32 rows [r0, r0 + 32) of an n x n matrix, column `col`, into registers.
// Rows and columns past n are clamped to n - 1, not predicated (a guard per
// load compiles to a branch per load): what they fetch is finite and meets a
// zero of the k slabs.
__device__ __forceinline__ void mt_load_half(float (&buf)[MT_HALF],
                                             const float* __restrict__ ws,
                                             int r0, int col, int n) {
  const int cc = min(col, n - 1);
  // The 64 row offsets of a tile do not change from matrix to matrix;
  // hoisted out of a loop over matrices they overflow the scalar registers.
  // An opaque copy of n makes every call work its own out, next to the loads
  // that use them.
  int nn = n;
  __asm__ volatile("" : "+s"(nn));
#pragma unroll
  for (int u = 0; u < MT_HALF; ++u) {
    buf[u] = ws[(long)min(r0 + u, nn - 1) * nn + cc];
  }
}

// acc[qq] += sum_u k_i[candidate 8 wave + qq][h0 + u] * buf[u].
__device__ __forceinline__ MT_NOPK void mt_fma_half(
    float (&acc)[MT_QW], const float (&buf)[MT_HALF], const float* ki_w) {
#pragma unroll
  for (int u = 0; u < MT_HALF; ++u) {
    // Nothing crosses this: left alone, the scheduler issues all 64 LDS
    // reads of a half before the first FMA and spills what they return.
    if (u % 4 == 0) __builtin_amdgcn_sched_barrier(0);
    const float4* k4 = reinterpret_cast<const float4*>(ki_w + u * MT_KLD);
    const float4 ka = k4[0], kb = k4[1];
    const float kv[MT_QW] = {ka.x, ka.y, ka.z, ka.w, kb.x, kb.y, kb.z, kb.w};
#pragma unroll
    for (int qq = 0; qq < MT_QW; ++qq) acc[qq] = fmaf(kv[qq], buf[u], acc[qq]);
  }
}
