// Fused posterior scorer for a group of Matern-5/2 GPs (gfx950): the uniform
// mixture of an ensemble's members (gp_model.EnsembleGPPosterior) and the
// transfer-learning stack (transfer_learning.StackedResidualGP.levels()).
//
// Numeric spec. Member g of G <= 8 has x_g (N_g, D), ls_g (D), amp_g, mean_g,
// alpha_g (N_g) and W_g (N_g, N_g) = K_g^-1:
//   k_g[n] = amp_g^2 m52(|(xq - x_g[n]) / ls_g|)
//   m_g    = mean_g + k_g . alpha_g
//   v_g    = max(amp_g^2 - k_g^T W_g k_g, 1e-12)
//   mean   = sum_g a_g m_g
//   var    = max(sum_g w_g v_g + c sum_g a_g (m_g - mean)^2, 1e-12)
//   dist   = min_n max_{d not one-hot} |xq_d - x_0[n, d]|     (member 0 only)
// Mixture: a_g = w_g = 1/G, c = 1 (mean of variances plus variance of means,
// never E[m^2] - E[m]^2). Stack: a_g = 1, c = 0, w_g the product of the dof
// factors down the chain. a, w, c are host floats.
//
// CONTRACT: every W_g must be EXACTLY symmetric. The quadform reads only the
// tile pairs ti <= tj and counts the off-diagonal ones twice.
//
// The ragged operands travel in one GrpArgs struct passed by value as a kernel
// argument (per-member pointers, sizes, prefix sums, scalars, run bounds): no
// device-side pointer table, no H2D copy, so the op is hipGraph-capturable.
//
// Three kernels, no atomics, every sum in one fixed order:
//  - grp_kvec_kernel: a work item is an x-run x a 64-row tile x 32 candidates.
//    An x-run is a maximal block of consecutive members with the same x
//    pointer and N (the whole ensemble; one member of a stack). The X tile is
//    staged transposed through LDS in 64-column chunks (lane = row, as
//    mt_kvec_kernel does) ONCE and serves every member of the run: one d2
//    accumulator per (member, candidate), the member's 1/ls a uniform scalar.
//    Writes k_g into the (b, sum N_g) workspace at the member's column offset,
//    the per-tile mean partials, and (run 0 only) member 0's L-inf partials.
//  - grp_quadform_kernel: the upper-triangular 64 x 64 tile pairs of ALL
//    members form one flat item list (per-member prefix in GrpArgs), walked
//    with a capped grid stride, so G small quadforms fill the chip together.
//    Per item the k_i / k_j slabs of the 32 candidates sit in LDS and the W_g
//    tile streams through two 32-row register buffers (mt_tile.h); the second
//    half's loads are issued before the first half's FMAs.
//  - grp_finalize_kernel: one wave per candidate; per member lane-strided
//    sums of the partials and a shuffle tree, then m_g, v_g, the combine, the
//    acquisition and the trust region.
// gfx950 has no fp32 MFMA and the quadform is subtracted from amp^2, so
// everything stays fp32 on the vector ALU.

#include <hip/hip_runtime.h>
#include "common.h"
#include "mt_tile.h"

#define GRP_GMAX 8

struct GrpArgs {
  const float* x[GRP_GMAX];
  const float* inv_ls[GRP_GMAX];
  const float* alpha[GRP_GMAX];
  const float* w[GRP_GMAX];
  int n[GRP_GMAX];
  int koff[GRP_GMAX];              // member's first column of the k workspace
  int tile_pre[GRP_GMAX + 1];      // 64-row tiles before member g
  int item_pre[GRP_GMAX + 1];      // quadform items before member g
  int run_first[GRP_GMAX + 1];     // first member of x-run r; [runs] = g
  int run_tile_pre[GRP_GMAX + 1];  // kvec tiles before x-run r
  float amp2[GRP_GMAX], mean[GRP_GMAX], a[GRP_GMAX], wt[GRP_GMAX];
  float c;
  int g, runs, ksum;
};
static_assert(sizeof(GrpArgs) < 4096, "kernel argument");

static int grp_tiles(int n) { return (n + MT_ROWS - 1) / MT_ROWS; }

extern "C" __global__ __launch_bounds__(MT_BLOCK) MT_NOPK void
grp_kvec_kernel(const float* __restrict__ xq,              // (B, D)
                const unsigned char* __restrict__ onehot,  // (D,)
                float* __restrict__ k_out,      // (B, ksum)
                float* __restrict__ mu_part,    // (B, tile_pre[g])
                float* __restrict__ dist_part,  // (B, tile_pre[1])
                int b, int d, const GrpArgs args) {
  __shared__ float x_t[MT_COLS * MT_LD];
  __shared__ __attribute__((aligned(16))) float xq_s[MT_COLS * MT_Q];

  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  int run = 0;
#pragma unroll
  for (int r = 1; r < GRP_GMAX; ++r) {
    if (r < args.runs && (int)blockIdx.x >= args.run_tile_pre[r]) run = r;
  }
  const int m0 = args.run_first[run];
  const int len = args.run_first[run + 1] - m0;
  const int tile = blockIdx.x - args.run_tile_pre[run];
  const float* __restrict__ x = args.x[m0];
  const int n = args.n[m0];
  const bool tr = run == 0;  // member 0 is in run 0
  const int row0 = tile * MT_ROWS;
  const int q0 = blockIdx.y * MT_Q;
  const int row = row0 + lane;
  const bool row_ok = row < n;

  // Uniform per-member pointers; the slots past the run repeat its last
  // member and are never read.
  const float* il[GRP_GMAX];
#pragma unroll
  for (int mm = 0; mm < GRP_GMAX; ++mm) {
    il[mm] = args.inv_ls[m0 + min(mm, len - 1)];
  }

  float d2[GRP_GMAX][MT_QW], linf[MT_QW];
#pragma unroll
  for (int qq = 0; qq < MT_QW; ++qq) {
    linf[qq] = 0.0f;
#pragma unroll
    for (int mm = 0; mm < GRP_GMAX; ++mm) d2[mm][qq] = 0.0f;
  }

  for (int c0 = 0; c0 < d; c0 += MT_COLS) {
    const int clen = min(MT_COLS, d - c0);
    // Rows past n read as zeros; their results are masked below.
    for (int e = tid; e < MT_ROWS * clen; e += MT_BLOCK) {
      const int r = e / clen, c = e - r * clen;
      const int rr = row0 + r;
      x_t[c * MT_LD + r] = rr < n ? x[(long)rr * d + c0 + c] : 0.0f;
    }
    // Wave w's candidates w, w + 4, ... sit side by side. Candidates past b
    // are zeros and never written back.
    for (int e = tid; e < MT_Q * clen; e += MT_BLOCK) {
      const int ql = e / clen, c = e - ql * clen;
      const int q = q0 + ql;
      const int slot = (ql % MT_WAVES) * MT_QW + ql / MT_WAVES;
      xq_s[c * MT_Q + slot] = q < b ? xq[(long)q * d + c0 + c] : 0.0f;
    }
    __syncthreads();

    for (int c = 0; c < clen; ++c) {
      const float xv = x_t[c * MT_LD + lane];
      const bool cont = tr && onehot[c0 + c] == 0;  // uniform branch
      const float4* xq4 =
          reinterpret_cast<const float4*>(&xq_s[c * MT_Q + wave * MT_QW]);
      const float4 xa = xq4[0], xb = xq4[1];
      const float diff[MT_QW] = {xa.x - xv, xa.y - xv, xa.z - xv, xa.w - xv,
                                 xb.x - xv, xb.y - xv, xb.z - xv, xb.w - xv};
      if (cont) {
#pragma unroll
        for (int qq = 0; qq < MT_QW; ++qq) {
          linf[qq] = fmaxf(linf[qq], fabsf(diff[qq]));
        }
      }
#pragma unroll
      for (int mm = 0; mm < GRP_GMAX; ++mm) {
        if (mm >= len) break;                // uniform
        const float s = il[mm][c0 + c];      // uniform: scalar load
#pragma unroll
        for (int qq = 0; qq < MT_QW; ++qq) {
          const float t = diff[qq] * s;
          d2[mm][qq] = fmaf(t, t, d2[mm][qq]);
        }
      }
    }
    __syncthreads();
  }

  const long tiles_all = args.tile_pre[args.g];
#pragma unroll
  for (int mm = 0; mm < GRP_GMAX; ++mm) {
    if (mm >= len) break;  // uniform
    const int m = m0 + mm;
    const float amp2 = args.amp2[m];
    const float al = row_ok ? args.alpha[m][row] : 0.0f;
    float* __restrict__ kcol = k_out + args.koff[m];
    const int slot = args.tile_pre[m] + tile;
#pragma unroll
    for (int qq = 0; qq < MT_QW; ++qq) {
      const int q = q0 + wave + qq * MT_WAVES;  // wave-uniform
      const float kv = row_ok ? amp2 * matern52_of_d2(d2[mm][qq]) : 0.0f;
      if (row_ok && q < b) kcol[(long)q * args.ksum + row] = kv;
      const float mu = wave_reduce_sum(kv * al);
      if (lane == 0 && q < b) mu_part[q * tiles_all + slot] = mu;
    }
  }
  if (tr) {
    const long tiles0 = args.tile_pre[1];
#pragma unroll
    for (int qq = 0; qq < MT_QW; ++qq) {
      const int q = q0 + wave + qq * MT_WAVES;
      const float dist = wave_reduce_min(row_ok ? linf[qq] : INFINITY);
      if (lane == 0 && q < b) dist_part[q * tiles0 + tile] = dist;
    }
  }
}

extern "C" __global__ __launch_bounds__(MT_BLOCK) MT_NOPK void
grp_quadform_kernel(const float* __restrict__ k,  // (B, ksum)
                    float* __restrict__ part,     // (B, item_pre[g])
                    int b, const GrpArgs args) {
  __shared__ __attribute__((aligned(16))) float ki_s[MT_ROWS * MT_KLD];
  __shared__ float kj_s[MT_Q * MT_ROWS];

  const int tid = threadIdx.x;
  const int wave = tid / WAVE_SIZE;
  const int lane = tid % WAVE_SIZE;
  const int q0 = blockIdx.y * MT_Q;
  const int items = args.item_pre[args.g];

  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    int m = 0;
#pragma unroll
    for (int g = 1; g < GRP_GMAX; ++g) {
      if (g < args.g && item >= args.item_pre[g]) m = g;
    }
    // Opaque and scalar: the member's operands are then fetched by indexed
    // scalar loads, not selected out of all eight members' values.
    __asm__ volatile("" : "+s"(m));
    const int n = args.n[m];
    const int tiles_n = (n + MT_ROWS - 1) / MT_ROWS;
    const float* __restrict__ w = args.w[m];
    const float* __restrict__ km = k + args.koff[m];
    // item -> (ti, tj), row-major over the member's upper triangle.
    int ti = 0, rem = item - args.item_pre[m];
    while (rem >= tiles_n - ti) {
      rem -= tiles_n - ti;
      ++ti;
    }
    const int tj = ti + rem;
    const int i0 = ti * MT_ROWS, j0 = tj * MT_ROWS;

    for (int e = tid; e < MT_Q * MT_ROWS; e += MT_BLOCK) {
      const int ql = e / MT_ROWS, c = e % MT_ROWS;
      const int q = q0 + ql;
      const float* kq = km + (long)q * args.ksum;
      ki_s[c * MT_KLD + ql] = (q < b && i0 + c < n) ? kq[i0 + c] : 0.0f;
      kj_s[e] = (q < b && j0 + c < n) ? kq[j0 + c] : 0.0f;
    }
    __syncthreads();

    const int col = j0 + lane;
    const float weight = ti == tj ? 1.0f : 2.0f;
    float wa[MT_HALF], wb[MT_HALF], acc[MT_QW];
#pragma unroll
    for (int qq = 0; qq < MT_QW; ++qq) acc[qq] = 0.0f;
    // An offset the compiler cannot see through: otherwise the k_i slab's
    // 128 LDS reads are all issued up front and held in registers.
    int ko = wave * MT_QW;
    __asm__ volatile("" : "+v"(ko));
    const float* ki_w = ki_s + ko;
    mt_load_half(wa, w, i0, col, n);
    mt_load_half(wb, w, i0 + MT_HALF, col, n);
    mt_fma_half(acc, wa, ki_w);
    // Pin the FMAs here, ahead of the second half's LDS reads.
    __asm__ volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]),
                          "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]),
                          "+v"(acc[6]), "+v"(acc[7]));
    mt_fma_half(acc, wb, ki_w + MT_HALF * MT_KLD);
    __asm__ volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]),
                          "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]),
                          "+v"(acc[6]), "+v"(acc[7]));
#pragma unroll
    for (int qq = 0; qq < MT_QW; ++qq) {
      const int ql = wave * MT_QW + qq;
      const float v = wave_reduce_sum(acc[qq] * kj_s[ql * MT_ROWS + lane]);
      if (lane == 0 && q0 + ql < b) {
        part[(long)(q0 + ql) * items + item] = weight * v;
      }
    }
    __syncthreads();  // the slabs are restaged on the next trip
  }
}

// One wave per candidate. Per member, lane l sums partials l, l + 64, ... in
// index order, then a shuffle tree: one fixed order, identical from run to
// run. score != NULL writes the score alone; otherwise (mean, sd, dist).
extern "C" __global__ __launch_bounds__(WAVE_SIZE) MT_NOPK void
grp_finalize_kernel(const float* __restrict__ part,       // (B, items)
                    const float* __restrict__ mu_part,    // (B, tiles)
                    const float* __restrict__ dist_part,  // (B, tiles of 0)
                    float* __restrict__ score, float* __restrict__ mean_out,
                    float* __restrict__ sd_out, float* __restrict__ dist_out,
                    int acq, float coef, float best_value, float tr_radius,
                    const GrpArgs args) {
  const int q = blockIdx.x;
  const int lane = threadIdx.x;
  const long items = args.item_pre[args.g], tiles = args.tile_pre[args.g];
  float mg[GRP_GMAX], vg[GRP_GMAX];
#pragma unroll
  for (int g = 0; g < GRP_GMAX; ++g) {
    mg[g] = 0.0f;
    vg[g] = 0.0f;
    if (g < args.g) {  // uniform
      const float* pp = part + q * items;
      const float* mp = mu_part + q * tiles;
      float v = 0.0f, u = 0.0f;
      for (int i = args.item_pre[g] + lane; i < args.item_pre[g + 1];
           i += WAVE_SIZE) {
        v += pp[i];
      }
      for (int i = args.tile_pre[g] + lane; i < args.tile_pre[g + 1];
           i += WAVE_SIZE) {
        u += mp[i];
      }
      mg[g] = args.mean[g] + wave_reduce_sum(u);
      vg[g] = fmaxf(args.amp2[g] - wave_reduce_sum(v), 1e-12f);
    }
  }
  const int tiles0 = args.tile_pre[1];
  float dist = INFINITY;
  for (int i = lane; i < tiles0; i += WAVE_SIZE) {
    dist = fminf(dist, dist_part[(long)q * tiles0 + i]);
  }
  dist = wave_reduce_min(dist);
  if (lane != 0) return;

  float mean = 0.0f;
#pragma unroll
  for (int g = 0; g < GRP_GMAX; ++g) {
    if (g < args.g) mean = fmaf(args.a[g], mg[g], mean);
  }
  float var = 0.0f, spread = 0.0f;
#pragma unroll
  for (int g = 0; g < GRP_GMAX; ++g) {
    if (g < args.g) {
      const float dm = mg[g] - mean;
      var = fmaf(args.wt[g], vg[g], var);
      spread = fmaf(args.a[g] * dm, dm, spread);
    }
  }
  const float sd = sqrtf(fmaxf(fmaf(args.c, spread, var), 1e-12f));
  if (score != nullptr) {
    score[q] = vz_trust_region(
        vz_acq_score(acq, mean, sd, coef, best_value), dist, tr_radius);
  } else {
    mean_out[q] = mean;
    sd_out[q] = sd;
    dist_out[q] = dist;
  }
}

// Workspace extents of a group: columns of k, mean-partial tiles, quadform
// items.
extern "C" void grp_layout(int g, const int* n, int* ksum, int* tiles,
                           int* items) {
  *ksum = *tiles = *items = 0;
  for (int i = 0; i < g; ++i) {
    const int t = grp_tiles(n[i]);
    *ksum += n[i];
    *tiles += t;
    *items += t * (t + 1) / 2;
  }
}

// score != NULL: scores (b,); otherwise mean_out, sd_out, dist_out (b,).
// The caller has checked 1 <= g <= 8 and every shape.
extern "C" void launch_grp(
    const float* xq, const unsigned char* onehot, int g,
    const float* const* x, const float* const* inv_ls,
    const float* const* alpha, const float* const* w, const int* n,
    const float* amp2, const float* mean, const float* a, const float* wt,
    float c, float* k_ws, float* part, float* mu_part, float* dist_part,
    float* score, float* mean_out, float* sd_out, float* dist_out, int b,
    int d, int acq, float coef, float best_value, float tr_radius,
    hipStream_t stream) {
  GrpArgs args = {};
  args.g = g;
  args.c = c;
  for (int i = 0; i < g; ++i) {
    const int t = grp_tiles(n[i]);
    args.x[i] = x[i];
    args.inv_ls[i] = inv_ls[i];
    args.alpha[i] = alpha[i];
    args.w[i] = w[i];
    args.n[i] = n[i];
    args.amp2[i] = amp2[i];
    args.mean[i] = mean[i];
    args.a[i] = a[i];
    args.wt[i] = wt[i];
    args.koff[i] = args.ksum;
    args.ksum += n[i];
    args.tile_pre[i + 1] = args.tile_pre[i] + t;
    args.item_pre[i + 1] = args.item_pre[i] + t * (t + 1) / 2;
    if (i == 0 || x[i] != x[i - 1] || n[i] != n[i - 1]) {  // a new x-run
      args.run_first[args.runs] = i;
      args.run_tile_pre[args.runs + 1] = args.run_tile_pre[args.runs] + t;
      ++args.runs;
    }
  }
  // The prefixes past the last member / run repeat the totals, so the
  // kernels' static [g + 1] reads stay defined.
  for (int i = g; i < GRP_GMAX; ++i) {
    args.tile_pre[i + 1] = args.tile_pre[g];
    args.item_pre[i + 1] = args.item_pre[g];
  }
  args.run_first[args.runs] = g;
  const int items = args.item_pre[g];
  const int groups = (b + MT_Q - 1) / MT_Q;
  hipLaunchKernelGGL(grp_kvec_kernel,
                     dim3(args.run_tile_pre[args.runs], groups),
                     dim3(MT_BLOCK), 0, stream, xq, onehot, k_ws, mu_part,
                     dist_part, b, d, args);
  hipLaunchKernelGGL(grp_quadform_kernel,
                     dim3(items < MT_GRID_MAX ? items : MT_GRID_MAX, groups),
                     dim3(MT_BLOCK), 0, stream, k_ws, part, b, args);
  hipLaunchKernelGGL(grp_finalize_kernel, dim3(b), dim3(WAVE_SIZE), 0, stream,
                     part, mu_part, dist_part, score, mean_out, sd_out,
                     dist_out, acq, coef, best_value, tr_radius, args);
}
