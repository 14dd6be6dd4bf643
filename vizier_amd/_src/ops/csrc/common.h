// Shared helpers for the vizier_amd CDNA4 (gfx950) kernels.
#pragma once

#include <hip/hip_runtime.h>

#define WAVE_SIZE 64

// Per-precision math for code templated over float / double. float keeps
// the fast intrinsics the fp32 kernels have always used (exp -> __expf,
// log -> __logf); double gets the accurate libm routines.
template <typename T>
struct vz_math;

template <>
struct vz_math<float> {
  static __device__ __forceinline__ float fma(float a, float b, float c) {
    return fmaf(a, b, c);
  }
  static __device__ __forceinline__ float fmax(float a, float b) {
    return fmaxf(a, b);
  }
  static __device__ __forceinline__ float fmin(float a, float b) {
    return fminf(a, b);
  }
  static __device__ __forceinline__ float fabs(float a) { return fabsf(a); }
  static __device__ __forceinline__ float exp(float a) { return __expf(a); }
  static __device__ __forceinline__ float log(float a) { return __logf(a); }
  static __device__ __forceinline__ float log1p(float a) {
    return log1pf(a);
  }
  static __device__ __forceinline__ float sqrt(float a) { return sqrtf(a); }
};

template <>
struct vz_math<double> {
  static __device__ __forceinline__ double fma(double a, double b,
                                               double c) {
    return ::fma(a, b, c);
  }
  static __device__ __forceinline__ double fmax(double a, double b) {
    return ::fmax(a, b);
  }
  static __device__ __forceinline__ double fmin(double a, double b) {
    return ::fmin(a, b);
  }
  static __device__ __forceinline__ double fabs(double a) {
    return ::fabs(a);
  }
  static __device__ __forceinline__ double exp(double a) { return ::exp(a); }
  static __device__ __forceinline__ double log(double a) { return ::log(a); }
  static __device__ __forceinline__ double log1p(double a) {
    return ::log1p(a);
  }
  static __device__ __forceinline__ double sqrt(double a) {
    return ::sqrt(a);
  }
};

// k(r) = (1 + sqrt5*r + 5r^2/3) exp(-sqrt5*r), r = sqrt(d2). The two
// precisions are separate formulas on purpose: fp32 multiplies by 1/3 and
// uses the fast exp, fp64 divides by 3 and uses the correctly-rounded /
// <1 ulp double sqrt and exp.
__device__ __forceinline__ float matern52_of_d2(float d2) {
  const float r = sqrtf(fmaxf(d2, 0.0f));
  const float sr = 2.2360679774997896f * r;  // sqrt(5) * r
  return (1.0f + sr + sr * sr * (1.0f / 3.0f)) * __expf(-sr);
}
__device__ __forceinline__ double matern52_of_d2(double d2) {
  const double sr = 2.23606797749978969641 * sqrt(fmax(d2, 0.0));
  return (1.0 + sr + sr * sr / 3.0) * exp(-sr);
}

// Eight OCP e4m3 bytes (byte 0 = element 0) -> eight bf16, exactly: e4m3's
// four significant bits and its exponent range fit in bf16, so the high
// half of the fp32 image IS the value. The fp8 grams feed these to the bf16
// MFMA (same rate as the non-scaled fp8 one on gfx950): the fp8 MFMA sums
// its 32 products in a truncating internal format, measured up to 2^-12.4
// of the largest product per K-step low, which put coincident rows at
// d^2 ~ 3e-5 instead of 0. bf16 x bf16 products of these values are exact
// in fp32 and the bf16 MFMA accumulates them to fp32 accuracy.
typedef __attribute__((ext_vector_type(8))) short vz_bf16x8;
typedef __attribute__((ext_vector_type(2))) float vz_f32x2;

__device__ __forceinline__ vz_bf16x8 vz_e4m3x8_to_bf16x8(long q) {
  const int w[2] = {(int)q, (int)(q >> 32)};
  union {
    unsigned int u[4];
    vz_bf16x8 v;
  } out;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const vz_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], false);
    const vz_f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], true);
    out.u[2 * i] = (__float_as_uint(lo.x) >> 16) |
                   (__float_as_uint(lo.y) & 0xffff0000u);
    out.u[2 * i + 1] = (__float_as_uint(hi.x) >> 16) |
                       (__float_as_uint(hi.y) & 0xffff0000u);
  }
  return out.v;
}

// Wave-wide reductions over all 64 lanes.
__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
  for (int offset = WAVE_SIZE / 2; offset > 0; offset >>= 1) {
    v += __shfl_down(v, offset, WAVE_SIZE);
  }
  return v;
}

__device__ __forceinline__ float wave_reduce_min(float v) {
#pragma unroll
  for (int offset = WAVE_SIZE / 2; offset > 0; offset >>= 1) {
    v = fminf(v, __shfl_down(v, offset, WAVE_SIZE));
  }
  return v;
}

__device__ __forceinline__ float wave_reduce_max(float v) {
#pragma unroll
  for (int offset = WAVE_SIZE / 2; offset > 0; offset >>= 1) {
    v = fmaxf(v, __shfl_down(v, offset, WAVE_SIZE));
  }
  return v;
}

// Block-level reduction: up to 4 waves -> LDS -> wave 0. The shuffle tree
// and the LDS pass have a fixed shape, so the result is run-to-run
// deterministic.
template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, T* lds4, Op op, T init) {
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
  return v;  // valid in wave 0 lane 0
}

// Counter-based RNG (splitmix64 -> uniform/laplace). Shared by the
// standalone Eagle kernels and the persistent sweep megakernel so the
// two paths draw IDENTICAL streams for the same (seed, offset, idx).
__device__ __forceinline__ unsigned long long vz_splitmix64(
    unsigned long long z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

template <typename T>
__device__ __forceinline__ T vz_rng_uniform(unsigned long long seed,
                                            unsigned long long offset,
                                            unsigned int idx) {
  // 24 bits k -> (k + 0.5) 2^-24 in (0, 1]. Both precisions draw the same
  // k. In double the sum is exact (25 significant bits). In float it is
  // exact for k < 2^23, rounded to even above (two k share a value), and
  // k = 2^24 - 1 gives exactly 1.0f. Callers tolerate the endpoint: the
  // Laplace draw clamps |u - 0.5|, the refill takes min(c, size - 1).
  unsigned long long h = vz_splitmix64(seed ^ vz_splitmix64(offset ^ idx));
  return (T(h >> 40) + T(0.5)) * (T(1) / T(16777216));
}

template <typename T>
__device__ __forceinline__ T vz_rng_laplace(unsigned long long seed,
                                            unsigned long long offset,
                                            unsigned int idx) {
  using M = vz_math<T>;
  const T u = vz_rng_uniform<T>(seed, offset, idx) - T(0.5);
  const T a = M::fmin(M::fabs(u), T(0.499999));
  return (u >= T(0) ? T(-1) : T(1)) * M::log1p(T(-2) * a);
}

__device__ __forceinline__ float vz_normal_cdf(float z) {
  return 0.5f * erfcf(-z * 0.70710678118654752f);
}
__device__ __forceinline__ float vz_normal_pdf(float z) {
  return 0.3989422804014327f * __expf(-0.5f * z * z);
}
__device__ __forceinline__ double vz_normal_cdf(double z) {
  return 0.5 * erfc(-z * 0.70710678118654752440);
}
__device__ __forceinline__ double vz_normal_pdf(double z) {
  return 0.39894228040143267794 * exp(-0.5 * z * z);
}

// Acquisition codes of every scorer (ops/dispatch.py passes them through).
#define ACQ_UCB 0
#define ACQ_LCB 1
#define ACQ_EI 2
#define ACQ_PI 3
#define ACQ_MEAN 4
#define ACQ_STDDEV 5

template <typename T>
__device__ __forceinline__ T vz_acq_score(int acq, T mu, T sd, T coef,
                                          T best_value) {
  switch (acq) {
    case ACQ_LCB: return mu - coef * sd;
    case ACQ_EI: {
      const T z = (mu - best_value) / sd;
      return sd * (z * vz_normal_cdf(z) + vz_normal_pdf(z));
    }
    case ACQ_PI: return vz_normal_cdf((mu - best_value) / sd);
    case ACQ_MEAN: return mu;
    case ACQ_STDDEV: return sd;
    case ACQ_UCB:
    default: return mu + coef * sd;
  }
}

// Trust region: a candidate farther than tr_radius (min L-inf distance to
// the training points) scores -1e4 - dist. A radius outside (0, 0.5]
// switches the region off.
template <typename T>
__device__ __forceinline__ T vz_trust_region(T score, T dist, T tr_radius) {
  if (tr_radius > T(0) && tr_radius <= T(0.5) && dist > tr_radius) {
    return T(-1e4) - dist;
  }
  return score;
}

// ---- Shared 64x64-tile K^-1 quadform --------------------------------------
//
// partial[q] contribution of tile (ti,tj) to quad[q] = k_q^T Kinv k_q,
// computed for ALL candidates at once so Kinv is read ONCE per scorer
// call. The per-candidate streaming variant reads Kinv b times per
// iteration (100 MB at N=1000, B=25) and measured 32.6 us of a 58 us
// Eagle iteration (profiles/sweep_kernels_r2.txt). Requires b <= 32
// and blockDim.x == 256. Used VERBATIM (same float-op order) by both
// the standalone chunked scorer and the persistent sweep megakernel so
// the two paths stay bit-identical.
#define VZ_QF_TILE 64
#define VZ_QF_QMAX 32

template <typename LoadK, typename StoreP>
__device__ __forceinline__ void vz_quadform_tile(
    const float* __restrict__ kinv, int b, int n, int tile, int tiles_n,
    float* k_i_lds, float* k_j_lds, LoadK loadk, StoreP store,
    unsigned long long* prof = nullptr) {
  const int tid = threadIdx.x;
  const bool profme = (prof != nullptr && tid == 0);
  unsigned long long tq0 = profme ? wall_clock64() : 0;
  const int ti = tile / tiles_n, tj = tile % tiles_n;
  const int i0 = ti * VZ_QF_TILE, j0 = tj * VZ_QF_TILE;
  const int ilen = min(VZ_QF_TILE, n - i0);
  const int jlen = min(VZ_QF_TILE, n - j0);
  for (int e = tid; e < VZ_QF_QMAX * VZ_QF_TILE; e += 256) {
    const int q = e / VZ_QF_TILE, c = e % VZ_QF_TILE;
    k_i_lds[e] = (q < b && c < ilen) ? loadk((long)q * n + i0 + c)
                                     : 0.0f;
    k_j_lds[e] = (q < b && c < jlen) ? loadk((long)q * n + j0 + c)
                                     : 0.0f;
  }
  __syncthreads();
  if (profme) {
    const unsigned long long tq1 = wall_clock64();
    prof[0] += tq1 - tq0;
    tq0 = tq1;
  }
  // Wave w owns candidates [8w, 8w+8); lane = tile column j. Kinv rows
  // are read coalesced across lanes (the 4 waves share each row
  // segment through L2).
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  float acc[8];
#pragma unroll
  for (int qq = 0; qq < 8; ++qq) acc[qq] = 0.0f;
  if (lane < jlen) {
    if (ilen == VZ_QF_TILE) {
      // Full tile: batch the Kinv row loads 8 at a time so they are
      // all in flight together. The rolled one-load-per-iteration
      // form serializes 64 dependent L2 round-trips (~300 ns each),
      // which made phase B ~12 us per tile in the megakernel
      // (profiles: tools_sweep_phases.py). Same fma order per
      // candidate chain — results are bit-identical.
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
  __syncthreads();
  if (profme) prof[1] += wall_clock64() - tq0;
}
