// Python bindings for the vizier_amd gfx950 kernels (torch extension).

#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include <algorithm>
#include <cstdlib>
#include <string>

#include <hip/hip_runtime.h>

extern "C" void launch_gram_matern52(const float* x1, const float* x2,
                                     const float* inv_ls, float* out,
                                     int n, int m, int d, float amp2,
                                     int sym, hipStream_t stream);

extern "C" void launch_gram_matern52_batched(
    const float* x, const float* inv_ls, const float* amp2,
    const float* noise, float* kout, float* gout, int r, int n, int d,
    hipStream_t stream);

extern "C" void launch_gram_matern52_bf16(
    const unsigned short* z1, const unsigned short* z2, const float* n1,
    const float* n2, float* out, int n, int m, int dp, float amp2,
    hipStream_t stream);

extern "C" void launch_gram_matern52_bf16_tiled(
    const unsigned short* z1, const unsigned short* z2, const float* n1,
    const float* n2, float* out, int n, int m, int dp, float amp2,
    hipStream_t stream);

extern "C" void launch_posterior_score(
    const float* xq, const float* x, const float* inv_ls,
    const float* alpha, const float* kinv, const unsigned char* onehot,
    float* out, int b, int n, int d, float amp2, float mean_c, int acq,
    float coef, float best_value, float tr_radius, hipStream_t stream);

extern "C" void launch_gram_matern52_fp8(
    const unsigned char* z1, const unsigned char* z2, const float* n1,
    const float* n2, float* out, int n, int m, int dp, float amp2,
    float scale2, hipStream_t stream);

extern "C" void launch_gram_matern52_fp8_tiled(
    const unsigned char* z1, const unsigned char* z2, const float* n1,
    const float* n2, float* out, int n, int m, int dp, float amp2,
    float scale2, hipStream_t stream);

extern "C" void launch_posterior_score_chunked(
    const float* xq, const float* x, const float* inv_ls,
    const float* alpha, const float* kinv, const unsigned char* onehot,
    float* k_ws, float* mu_ws, float* dist_ws, float* var_ws, float* out,
    int b, int n, int d, float amp2, float mean_c, int acq, float coef,
    float best_value, float tr_radius, hipStream_t stream);

extern "C" void launch_ps_kvec(
    const float* xq, const float* x, const float* inv_ls,
    const float* alpha, const unsigned char* onehot, float* k_ws,
    float* mu_ws, float* dist_ws, int b, int n, int d, float amp2,
    hipStream_t stream);

extern "C" void launch_ps_kvec_split(
    const float* xq, const float* x, const float* inv_ls,
    const float* alpha, const unsigned char* onehot, float* k_ws,
    float* mu_part, float* dist_part, float* mu_ws, float* dist_ws,
    int b, int n, int d, float amp2, int rchunks, hipStream_t stream);

extern "C" void launch_ps_quadform_tile(
    const float* k_ws, const float* kinv, float* var_part, float* quad,
    int b, int n, hipStream_t stream);

extern "C" void launch_ps_quadform_big(
    const float* k_ws, const float* kinv, float* part, float* quad,
    int b, int n, hipStream_t stream);

extern "C" void launch_ps_kvec_fp8(
    const float* z1f, const float* n1, const float* xq, const float* x,
    const unsigned char* z2q, const float* n2, const float* alpha,
    const unsigned char* onehot, float* k_ws, float* mu_ws,
    float* dist_ws, int b, int n, int d, int dp, float amp2,
    float scale, hipStream_t stream);

extern "C" void launch_ps_finalize_meanstd(
    const float* mu_ws, const float* var_ws, float* mean_out,
    float* sd_out, int b, float amp2, float mean_c, int nchunk,
    hipStream_t stream);

extern "C" void launch_ps_finalize_meanstd_direct(
    const float* mu_ws, const float* quad, float* mean_out,
    float* sd_out, int b, float amp2, float mean_c,
    hipStream_t stream);

extern "C" void launch_hv_scalarize_tr(
    const float* means, const float* sds, const float* weights,
    const float* ref, const float* dist, float* out, int b, int m,
    int s, float coef, float tr_radius, hipStream_t stream);

extern "C" void launch_ps_quadform_kernel_only(
    const float* k_ws, const float* kinv, float* var_ws, int b, int n,
    hipStream_t stream);

extern "C" void launch_ps_finalize_direct(
    const float* mu_ws, const float* dist_ws, const float* quad,
    float* out, int b, float amp2, float mean_c, int acq, float coef,
    float best_value, float tr_radius, hipStream_t stream);

extern "C" void launch_ps_kvec_bf16(
    const float* xq, const float* x, const unsigned short* z2b,
    const float* n2, const float* inv_ls, const float* alpha,
    const unsigned char* onehot, float* k_ws, float* mu_ws,
    float* dist_ws, int b, int n, int d, int dp, float amp2,
    hipStream_t stream);

extern "C" void launch_ps_quadform_finalize(
    const float* k_ws, const float* kinv, const float* mu_ws,
    const float* dist_ws, float* var_ws, float* out, int b, int n,
    float amp2, float mean_c, int acq, float coef, float best_value,
    float tr_radius, hipStream_t stream);

extern "C" void launch_qei_cov(
    const float* t_ws, const float* k_ws, const float* mu_ws,
    const float* xs, const float* inv_ls, float* mean_out, float* cov_out,
    int b, int q, int n, int d, float amp2, float mean_c,
    hipStream_t stream);
extern "C" void launch_qei_mc(
    const float* mean, const float* cov, const float* eps,
    const float* dist, float* out, int b, int q, int s, float best_value,
    float tr_radius, hipStream_t stream);
extern "C" void launch_setpe_logdet(
    const float* cov, const float* mean, const float* sd, const float* dist,
    float* out, int b, int q, float jitter, float threshold,
    float explore_coef, float penalty_coef, float tr_radius,
    hipStream_t stream);
extern "C" int batched_potrf_panel_rows(int impl);
extern "C" int batched_potrf_needs_scratch(int n, int impl);
extern "C" void batched_potrf_launch_shape(int n, int impl, int out[2]);
extern "C" void launch_batched_potrf(float* A, int* info, float* dscratch,
                                     int r, int n, int impl,
                                     hipStream_t stream);
extern "C" void launch_batched_trsv_lower(const float* L, float* b,
                                          int r, int n, int variant,
                                          hipStream_t stream);

extern "C" void launch_eagle_suggest(
    const float* pool_cont, const long* pool_cat, const float* rewards,
    const float* perturbations, const long* cat_sizes, float* out_cont,
    long* out_cat, const unsigned long long* iter_ptr, int n_batches,
    int batch_size, int pool_size, int q,
    int dc, int dcat, int max_cat, float visibility, float gravity,
    float neg_gravity, float norm_scale, float cat_factor, float p_same,
    unsigned long long seed, hipStream_t stream);

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
    float tr_radius, hipStream_t stream);

extern "C" void launch_eagle_update(
    float* pool_cont, long* pool_cat, float* rewards, float* perturbations,
    const float* batch_cont, const long* batch_cat,
    const float* batch_rewards, const long* cat_sizes, float* best_reward,
    unsigned long long* iter_ptr, int n_batches, int batch_size, int q,
    int dc, int dcat,
    float penalize_factor, float perturbation_lower_bound,
    float base_perturbation, unsigned long long seed,
    hipStream_t stream);

// fp64 parity-mode kernels (posterior_score_f64.hip, gram_matern52_f64.hip,
// the double instantiations of eagle_step.hip).
extern "C" void ps_f64_quadform_shape(int n, int* ctiles, int* slabs,
                                      int* slab_rows);

extern "C" void launch_posterior_score_f64(
    const double* xq, const double* x, const double* inv_ls,
    const double* alpha, const double* kinv, const unsigned char* onehot,
    double* k_ws, double* mu_ws, double* dist_ws, double* part,
    double* out, double* mean_out, double* sd_out, int b, int n, int d,
    double amp2, double mean_c, int acq, double coef, double best_value,
    double tr_radius, hipStream_t stream);

extern "C" void launch_gram_matern52_f64(
    const double* x1, const double* x2, const double* inv_ls, double* out,
    int n, int m, int d, double amp2, int sym, hipStream_t stream);

extern "C" void launch_eagle_suggest_f64(
    const double* pool_cont, const long* pool_cat, const double* rewards,
    const double* perturbations, const long* cat_sizes, double* out_cont,
    long* out_cat, const unsigned long long* iter_ptr, int n_batches,
    int batch_size, int pool_size, int q, int dc, int dcat, int max_cat,
    double visibility, double gravity, double neg_gravity,
    double norm_scale, double cat_factor, double p_same,
    unsigned long long seed, hipStream_t stream);

extern "C" void launch_eagle_update_f64(
    double* pool_cont, long* pool_cat, double* rewards,
    double* perturbations, const double* batch_cont, const long* batch_cat,
    const double* batch_rewards, const long* cat_sizes,
    double* best_reward, unsigned long long* iter_ptr, int n_batches,
    int batch_size, int q, int dc, int dcat, double penalize_factor,
    double perturbation_lower_bound, double base_perturbation,
    unsigned long long seed, hipStream_t stream);

namespace {

torch::Tensor check_f32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be fp32");
  return t.contiguous();
}

hipStream_t current_stream() {
  return at::cuda::getCurrentCUDAStream().stream();
}

// Host-side argument checks shared by the fused scorer bindings. The
// kernels index x, alpha, kinv and onehot by (n, d) taken from xq/x
// alone, so every other operand must agree BEFORE anything is launched.
void check_scorer_args(const torch::Tensor& xq, const torch::Tensor& x,
                       const torch::Tensor& lengthscales,
                       const torch::Tensor& alpha,
                       const torch::Tensor& kinv,
                       const torch::Tensor& onehot) {
  TORCH_CHECK(xq.dim() == 2 && x.dim() == 2, "xq and x must be 2-D");
  const int64_t d = xq.size(1), n = x.size(0);
  TORCH_CHECK(x.size(1) == d, "x must have xq's ", d, " columns, got ",
              x.size(1));
  TORCH_CHECK(lengthscales.numel() == d, "lengthscales must have ", d,
              " elements, got ", lengthscales.numel());
  TORCH_CHECK(alpha.numel() == n, "alpha must have ", n,
              " elements, got ", alpha.numel());
  TORCH_CHECK(kinv.dim() == 2 && kinv.size(0) == n && kinv.size(1) == n,
              "kinv must be (", n, ", ", n, ")");
  TORCH_CHECK(onehot.scalar_type() == torch::kUInt8 && onehot.is_cuda(),
              "onehot must be a uint8 GPU tensor");
  TORCH_CHECK(onehot.numel() == d, "onehot must have ", d,
              " elements, got ", onehot.numel());
}

// Cached training-side operands (z2b / z2q rows, n2) of the bf16/fp8
// scorers must cover the same n training rows as x.
void check_cached_operands(const torch::Tensor& z2, const torch::Tensor& n2,
                           const torch::Tensor& x, const char* name) {
  TORCH_CHECK(z2.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(z2.dim() == 2 && z2.size(0) == x.size(0), name,
              " must have x's ", x.size(0), " rows");
  TORCH_CHECK(n2.numel() == x.size(0), "n2 must have ", x.size(0),
              " elements, got ", n2.numel());
}

// Shape checks shared by the gram bindings: the kernels index x1, x2 and
// the lengthscales by (n, m, d) taken from x1 and x2 alone, so the
// operands must agree BEFORE any size() read past dim() or any launch.
void check_gram_args(const torch::Tensor& x1, const torch::Tensor& x2,
                     const torch::Tensor& lengthscales) {
  TORCH_CHECK(x1.dim() == 2 && x2.dim() == 2,
              "x1 and x2 must be 2-D, got ", x1.dim(), "-D and ",
              x2.dim(), "-D");
  const int64_t d = x1.size(1);
  TORCH_CHECK(x2.size(1) == d, "x2 must have x1's ", d, " columns, got ",
              x2.size(1));
  TORCH_CHECK(lengthscales.numel() == d, "lengthscales must have ", d,
              " elements, got ", lengthscales.numel());
}

torch::Tensor gram_matern52(torch::Tensor x1, torch::Tensor x2,
                            torch::Tensor lengthscales, double amplitude) {
  x1 = check_f32(x1, "x1");
  x2 = check_f32(x2, "x2");
  lengthscales = check_f32(lengthscales, "lengthscales");
  check_gram_args(x1, x2, lengthscales);
  // The kernel indexes out[row * m + col] and x[row * d + c] in int.
  TORCH_CHECK(x1.size(0) * x2.size(0) < (int64_t(1) << 31) &&
              x1.numel() < (int64_t(1) << 31) &&
              x2.numel() < (int64_t(1) << 31),
              "gram_matern52 supports fewer than 2^31 elements in x1, x2 "
              "and the (", x1.size(0), ", ", x2.size(0), ") output");
  const int n = x1.size(0), m = x2.size(0), d = x1.size(1);
  auto out = torch::empty({n, m}, x1.options());
  if (n == 0 || m == 0) return out;
  auto inv_ls = 1.0f / lengthscales;
  const int sym = (x1.data_ptr() == x2.data_ptr() && n == m) ? 1 : 0;
  launch_gram_matern52(x1.data_ptr<float>(), x2.data_ptr<float>(),
                       inv_ls.data_ptr<float>(), out.data_ptr<float>(), n,
                       m, d, (float)(amplitude * amplitude), sym,
                       current_stream());
  return out;
}

std::vector<torch::Tensor> gram_matern52_batched(
    torch::Tensor x, torch::Tensor lengthscales, torch::Tensor amplitude,
    torch::Tensor noise, bool want_grad_factor) {
  // (N, D) x; (R, D) lengthscales; (R,) amplitude, noise. Returns
  // [K (R, N, N) with noise*I folded in] or [K, G] with the
  // Matern-5/2 gradient factor.
  x = check_f32(x, "x");
  lengthscales = check_f32(lengthscales, "lengthscales");
  amplitude = check_f32(amplitude, "amplitude");
  noise = check_f32(noise, "noise");
  TORCH_CHECK(x.dim() == 2, "x must be 2-D, got ", x.dim(), "-D");
  TORCH_CHECK(lengthscales.dim() == 2 &&
              lengthscales.size(1) == x.size(1),
              "lengthscales must be (R, D) with x's D");
  const int n = x.size(0), d = x.size(1);
  const int r = lengthscales.size(0);
  TORCH_CHECK(amplitude.numel() == r && noise.numel() == r,
              "amplitude/noise must be (R,)");
  // The kernel indexes x[row * d + c] in int and R rides on gridDim.y.
  TORCH_CHECK(x.numel() < (int64_t(1) << 31) && r <= 65535,
              "gram_matern52_batched supports fewer than 2^31 elements in "
              "x and R <= 65535");
  auto inv_ls = (1.0f / lengthscales).contiguous();
  auto amp2 = (amplitude * amplitude).contiguous();
  auto K = torch::empty({r, n, n}, x.options());
  torch::Tensor G;
  float* gptr = nullptr;
  if (want_grad_factor) {
    G = torch::empty({r, n, n}, x.options());
    gptr = G.data_ptr<float>();
  }
  if (n == 0 || r == 0) {
    if (want_grad_factor) return {K, G};
    return {K};
  }
  launch_gram_matern52_batched(
      x.data_ptr<float>(), inv_ls.data_ptr<float>(),
      amp2.data_ptr<float>(), noise.data_ptr<float>(),
      K.data_ptr<float>(), gptr, r, n, d, current_stream());
  if (want_grad_factor) return {K, G};
  return {K};
}

torch::Tensor gram_matern52_bf16_impl(torch::Tensor x1, torch::Tensor x2,
                                      torch::Tensor lengthscales,
                                      double amplitude, bool tiled) {
  x1 = check_f32(x1, "x1");
  x2 = check_f32(x2, "x2");
  lengthscales = check_f32(lengthscales, "lengthscales");
  check_gram_args(x1, x2, lengthscales);
  const int n = x1.size(0), m = x2.size(0), d = x1.size(1);
  if (n == 0 || m == 0) return torch::empty({n, m}, x1.options());
  auto z1 = x1 / lengthscales;
  // Same pointer is the same operand only when the row counts agree too:
  // x[:1] and x share a pointer, and a (1, d) z1 would be broadcast into
  // every row of z2b below.
  auto z2 = (x1.data_ptr() == x2.data_ptr() && n == m) ? z1
                                                       : x2 / lengthscales;
  const int dp = (d + 31) / 32 * 32;
  auto z1b = torch::zeros({n, dp},
                          x1.options().dtype(torch::kBFloat16));
  auto z2b = torch::zeros({m, dp},
                          x1.options().dtype(torch::kBFloat16));
  z1b.index_put_({torch::indexing::Slice(),
                  torch::indexing::Slice(0, d)}, z1.to(torch::kBFloat16));
  z2b.index_put_({torch::indexing::Slice(),
                  torch::indexing::Slice(0, d)}, z2.to(torch::kBFloat16));
  // Norms of the bf16-ROUNDED vectors: bf16 x bf16 products accumulate
  // exactly in fp32, so d^2 = n1 + n2 - 2 z1b.z2b is the exact squared
  // distance of the rounded inputs (diagonal exactly 0).
  auto n1 = (z1b.to(torch::kFloat32) * z1b.to(torch::kFloat32)).sum(-1);
  auto n2 = (z2b.to(torch::kFloat32) * z2b.to(torch::kFloat32)).sum(-1);
  auto out = torch::empty({n, m}, x1.options());
  auto launch = tiled ? launch_gram_matern52_bf16_tiled
                      : launch_gram_matern52_bf16;
  launch((const unsigned short*)z1b.data_ptr(),
         (const unsigned short*)z2b.data_ptr(), n1.data_ptr<float>(),
         n2.data_ptr<float>(), out.data_ptr<float>(), n, m, dp,
         (float)(amplitude * amplitude), current_stream());
  return out;
}

torch::Tensor gram_matern52_bf16(torch::Tensor x1, torch::Tensor x2,
                                 torch::Tensor lengthscales,
                                 double amplitude) {
  // LDS-tiled MFMA path once both dims fill 128x128 tiles; the
  // register-direct strip kernel has less overhead for small grams.
  const bool tiled = x1.dim() == 2 && x2.dim() == 2 &&
                     x1.size(0) >= 512 && x2.size(0) >= 512;
  return gram_matern52_bf16_impl(x1, x2, lengthscales, amplitude, tiled);
}

torch::Tensor gram_matern52_bf16_tiled(torch::Tensor x1, torch::Tensor x2,
                                       torch::Tensor lengthscales,
                                       double amplitude) {
  return gram_matern52_bf16_impl(x1, x2, lengthscales, amplitude, true);
}

torch::Tensor posterior_scores(torch::Tensor xq, torch::Tensor x,
                               torch::Tensor lengthscales, double amplitude,
                               double mean_c, torch::Tensor alpha,
                               torch::Tensor kinv, torch::Tensor onehot,
                               int64_t acq, double coef, double best_value,
                               double tr_radius) {
  xq = check_f32(xq, "xq");
  x = check_f32(x, "x");
  lengthscales = check_f32(lengthscales, "lengthscales");
  alpha = check_f32(alpha, "alpha");
  kinv = check_f32(kinv, "kinv");
  TORCH_CHECK(onehot.scalar_type() == torch::kUInt8 && onehot.is_cuda(),
              "onehot must be a uint8 GPU tensor");
  onehot = onehot.contiguous();
  const int b = xq.size(0), d = xq.size(1), n = x.size(0);
  TORCH_CHECK(d <= 512, "posterior_scores supports D <= 512");
  TORCH_CHECK(n <= 36000, "posterior_scores supports N <= 36000 (LDS)");
  TORCH_CHECK(x.size(1) == d && alpha.numel() == n &&
              kinv.size(0) == n && kinv.size(1) == n, "shape mismatch");
  auto inv_ls = 1.0f / lengthscales;
  auto out = torch::empty({b}, xq.options());
  launch_posterior_score(
      xq.data_ptr<float>(), x.data_ptr<float>(), inv_ls.data_ptr<float>(),
      alpha.data_ptr<float>(), kinv.data_ptr<float>(),
      onehot.data_ptr<unsigned char>(), out.data_ptr<float>(), b, n, d,
      (float)(amplitude * amplitude), (float)mean_c, (int)acq, (float)coef,
      (float)best_value, (float)tr_radius, current_stream());
  return out;
}

torch::Tensor gram_matern52_fp8_impl(torch::Tensor x1, torch::Tensor x2,
                                     torch::Tensor lengthscales,
                                     double amplitude, bool tiled) {
  x1 = check_f32(x1, "x1");
  x2 = check_f32(x2, "x2");
  lengthscales = check_f32(lengthscales, "lengthscales");
  check_gram_args(x1, x2, lengthscales);
  const int n = x1.size(0), m = x2.size(0), d = x1.size(1);
  if (n == 0 || m == 0) return torch::empty({n, m}, x1.options());
  auto z1 = x1 / lengthscales;
  // As in the bf16 binding: alias only when the row counts agree.
  auto z2 = (x1.data_ptr() == x2.data_ptr() && n == m) ? z1
                                                       : x2 / lengthscales;
  // Pre-scale into comfortable e4m3 range (|z|/s <= ~8).
  double s = std::max(z1.abs().max().item<double>(),
                      z2.abs().max().item<double>()) / 8.0;
  s = std::max(s, 1e-8);
  const int dp = (d + 31) / 32 * 32;
  auto opts8 = x1.options().dtype(torch::kFloat8_e4m3fn);
  auto z1b = torch::zeros({n, dp}, opts8);
  auto z2b = torch::zeros({m, dp}, opts8);
  z1b.index_put_({torch::indexing::Slice(),
                  torch::indexing::Slice(0, d)},
                 (z1 / s).to(torch::kFloat8_e4m3fn));
  z2b.index_put_({torch::indexing::Slice(),
                  torch::indexing::Slice(0, d)},
                 (z2 / s).to(torch::kFloat8_e4m3fn));
  auto z1f = z1b.to(torch::kFloat32) * s;
  auto z2f = z2b.to(torch::kFloat32) * s;
  auto n1 = (z1f * z1f).sum(-1);
  auto n2 = (z2f * z2f).sum(-1);
  auto out = torch::empty({n, m}, x1.options());
  auto launch = tiled ? launch_gram_matern52_fp8_tiled
                      : launch_gram_matern52_fp8;
  launch((const unsigned char*)z1b.data_ptr(),
         (const unsigned char*)z2b.data_ptr(), n1.data_ptr<float>(),
         n2.data_ptr<float>(), out.data_ptr<float>(), n, m, dp,
         (float)(amplitude * amplitude), (float)(s * s),
         current_stream());
  return out;
}

torch::Tensor gram_matern52_fp8(torch::Tensor x1, torch::Tensor x2,
                                torch::Tensor lengthscales,
                                double amplitude) {
  const bool tiled = x1.dim() == 2 && x2.dim() == 2 &&
                     x1.size(0) >= 512 && x2.size(0) >= 512;
  return gram_matern52_fp8_impl(x1, x2, lengthscales, amplitude, tiled);
}

torch::Tensor gram_matern52_fp8_tiled(torch::Tensor x1, torch::Tensor x2,
                                      torch::Tensor lengthscales,
                                      double amplitude) {
  return gram_matern52_fp8_impl(x1, x2, lengthscales, amplitude, true);
}

namespace {

// Large-N variance quadform: ONE rocBLAS/hipBLASLt SGEMM by default.
// The hand-written split-K column-owner kernel (ps_quadform_big) is
// the VIZIER_AMD_QUADFORM=custom opt-in: it reads Kinv exactly once
// with perfect coalescing but measured 0.445 ms vs the library's
// 0.263 ms at (b=25, N=10^4) — the library's tiling wins this skinny
// shape (profiles/quadform_ab_r2.json); both are ~5x off the 50 us
// HBM floor, so the kernel stays for future split-K work.
// Small/medium-N quadform: the 64x64-tile kernel reads Kinv ONCE per
// call (vs once per candidate in the legacy chunked kernel — 32.6 us
// of a 58 us Eagle iteration at N=1000, profiles/sweep_kernels_r2.txt).
// b <= 32 only; returns the (b,) quadform.
torch::Tensor quadform_tile_small_n(const torch::Tensor& k_ws,
                                    const torch::Tensor& kinv, int b,
                                    int n, hipStream_t stream) {
  const int tiles_n = (n + 63) / 64;
  const long total = (long)tiles_n * tiles_n;
  auto var_part = torch::empty({b, total}, k_ws.options());
  auto quad = torch::empty({b}, k_ws.options());
  launch_ps_quadform_tile(k_ws.data_ptr<float>(),
                          kinv.data_ptr<float>(),
                          var_part.data_ptr<float>(),
                          quad.data_ptr<float>(), b, n, stream);
  return quad;
}

torch::Tensor quadform_large_n(const torch::Tensor& k_ws,
                               const torch::Tensor& kinv, int b, int n,
                               hipStream_t stream) {
  static const bool force_custom = []() {
    const char* s = getenv("VIZIER_AMD_QUADFORM");
    return s && std::string(s) == "custom";
  }();
  if (force_custom && b <= 32) {
    const int jchunks = (n + 255) / 256;
    int ichunks = (512 + jchunks - 1) / jchunks;
    if (ichunks < 1) ichunks = 1;
    auto part = torch::empty({b, (long)jchunks * ichunks},
                             k_ws.options());
    auto quad = torch::empty({b}, k_ws.options());
    launch_ps_quadform_big(k_ws.data_ptr<float>(),
                           kinv.data_ptr<float>(),
                           part.data_ptr<float>(),
                           quad.data_ptr<float>(), b, n, stream);
    return quad;
  }
  auto t = at::matmul(k_ws, kinv);
  return (k_ws * t).sum(-1);
}

// -- Pieces of the fused scorer pipeline ---------------------------------
//
// posterior_scores_chunked, posterior_scores_bf16, posterior_mean_std and
// posterior_mean_std_fp8 all run: k-vector kernel -> quadform by one of
// three routes -> finalize.

// Large-N quadform via one rocBLAS SGEMM: K_inv is read ONCE per
// iteration instead of once per candidate (the per-candidate streaming
// path moves b * N^2 * 4 bytes of HBM per call — 10 GB at N=10^4, B=25 —
// and measured 4.2 ms/iter on BASELINE config 4). Crossover default 4096
// (below that K_inv is L2/MALL-resident and the fused kernels win on
// launch count); override with VIZIER_AMD_PS_GEMM_N.
int gemm_n_threshold() {
  static const int threshold = []() {
    const char* s = getenv("VIZIER_AMD_PS_GEMM_N");
    return s ? atoi(s) : 4096;
  }();
  return threshold;
}

enum class QuadRoute { kGemm, kTile, kLegacy };

QuadRoute quad_route(int n, int b) {
  if (n >= gemm_n_threshold()) return QuadRoute::kGemm;
  return b <= 32 ? QuadRoute::kTile : QuadRoute::kLegacy;
}

// What every k-vector kernel writes: k (b, n), mu (b,) without the mean
// constant, dist (b,) min L-inf distance to the training points.
struct ScorerWs {
  torch::Tensor k, mu, dist;
  ScorerWs(const torch::Tensor& xq, int n)
      : k(torch::empty({xq.size(0), n}, xq.options())),
        mu(torch::empty({xq.size(0)}, xq.options())),
        dist(torch::empty({xq.size(0)}, xq.options())) {}
};

struct AcqArgs {
  float amp2, mean_c;
  int acq;
  float coef, best_value, tr_radius;
};

// The fp32 k-vector: one workgroup per candidate, or the row-split
// variant that fills the chip at large N.
void kvec_f32(const torch::Tensor& xq, const torch::Tensor& x,
              const torch::Tensor& inv_ls, const torch::Tensor& alpha,
              const torch::Tensor& onehot, ScorerWs& ws, float amp2,
              bool split) {
  const int b = xq.size(0), d = xq.size(1), n = x.size(0);
  if (!split) {
    launch_ps_kvec(
        xq.data_ptr<float>(), x.data_ptr<float>(),
        inv_ls.data_ptr<float>(), alpha.data_ptr<float>(),
        onehot.data_ptr<unsigned char>(), ws.k.data_ptr<float>(),
        ws.mu.data_ptr<float>(), ws.dist.data_ptr<float>(), b, n, d, amp2,
        current_stream());
    return;
  }
  const int rchunks = std::max(1, 512 / std::max(b, 1));
  auto mu_part = torch::empty({b, rchunks}, xq.options());
  auto dist_part = torch::empty({b, rchunks}, xq.options());
  launch_ps_kvec_split(
      xq.data_ptr<float>(), x.data_ptr<float>(), inv_ls.data_ptr<float>(),
      alpha.data_ptr<float>(), onehot.data_ptr<unsigned char>(),
      ws.k.data_ptr<float>(), mu_part.data_ptr<float>(),
      dist_part.data_ptr<float>(), ws.mu.data_ptr<float>(),
      ws.dist.data_ptr<float>(), b, n, d, amp2, rchunks, current_stream());
}

// The (b,) quadform by the GEMM or the tile route. The legacy NCHUNK
// route has no common form: each binding has its own launcher for it.
torch::Tensor quadform(QuadRoute route, const ScorerWs& ws,
                       const torch::Tensor& kinv) {
  const int b = ws.k.size(0), n = ws.k.size(1);
  return route == QuadRoute::kTile
      ? quadform_tile_small_n(ws.k, kinv, b, n, current_stream())
      : quadform_large_n(ws.k, kinv, b, n, current_stream());
}

torch::Tensor finalize_score(const ScorerWs& ws, const torch::Tensor& quad,
                             const AcqArgs& a) {
  const int b = ws.mu.size(0);
  auto out = torch::empty({b}, ws.mu.options());
  launch_ps_finalize_direct(
      ws.mu.data_ptr<float>(), ws.dist.data_ptr<float>(),
      quad.data_ptr<float>(), out.data_ptr<float>(), b, a.amp2, a.mean_c,
      a.acq, a.coef, a.best_value, a.tr_radius, current_stream());
  return out;
}

// var is the (b,) quadform (nchunk == 0) or (b, nchunk) partial sums.
std::vector<torch::Tensor> finalize_meanstd(const ScorerWs& ws,
                                            const torch::Tensor& var,
                                            int nchunk, float amp2,
                                            float mean_c) {
  const int b = ws.mu.size(0);
  auto mean = torch::empty({b}, ws.mu.options());
  auto sd = torch::empty({b}, ws.mu.options());
  if (nchunk == 0) {
    launch_ps_finalize_meanstd_direct(
        ws.mu.data_ptr<float>(), var.data_ptr<float>(),
        mean.data_ptr<float>(), sd.data_ptr<float>(), b, amp2, mean_c,
        current_stream());
  } else {
    launch_ps_finalize_meanstd(
        ws.mu.data_ptr<float>(), var.data_ptr<float>(),
        mean.data_ptr<float>(), sd.data_ptr<float>(), b, amp2, mean_c,
        nchunk, current_stream());
  }
  return {mean, sd, ws.dist};
}

constexpr int kLegacyNchunk = 10;  // NCHUNK of posterior_score.hip

}  // namespace

torch::Tensor gram_matern52_fp8_pre(
    torch::Tensor z1q, torch::Tensor z2q, torch::Tensor n1,
    torch::Tensor n2, double amplitude, double scale) {
  // Cross-gram from PRE-QUANTIZED fp8 operands: the per-call
  // host-side range scan (.item() sync) and conversions of the
  // training side are hoisted out by the caller (once per suggest),
  // so this is one launch and stream-capture-safe.
  TORCH_CHECK(z1q.scalar_type() == torch::kFloat8_e4m3fn &&
              z2q.scalar_type() == torch::kFloat8_e4m3fn,
              "z1q/z2q must be float8_e4m3fn");
  TORCH_CHECK(z1q.is_cuda() && z2q.is_cuda(),
              "z1q/z2q must be GPU tensors");
  TORCH_CHECK(z1q.dim() == 2 && z2q.dim() == 2,
              "z1q and z2q must be 2-D, got ", z1q.dim(), "-D and ",
              z2q.dim(), "-D");
  z1q = z1q.contiguous();
  z2q = z2q.contiguous();
  n1 = check_f32(n1, "n1");
  n2 = check_f32(n2, "n2");
  const int n = z1q.size(0), m = z2q.size(0), dp = z1q.size(1);
  TORCH_CHECK(z2q.size(1) == dp && dp % 32 == 0,
              "z1q and z2q must share a column count that is a multiple "
              "of 32, got ", dp, " and ", z2q.size(1));
  // The kernel indexes n1 and n2 by n and m.
  TORCH_CHECK(n1.numel() == n, "n1 must have ", n, " elements, got ",
              n1.numel());
  TORCH_CHECK(n2.numel() == m, "n2 must have ", m, " elements, got ",
              n2.numel());
  auto out = torch::empty({n, m},
                          n1.options().dtype(torch::kFloat32));
  if (n == 0 || m == 0) return out;
  const bool tiled = n >= 512 && m >= 512;
  auto launch = tiled ? launch_gram_matern52_fp8_tiled
                      : launch_gram_matern52_fp8;
  launch((const unsigned char*)z1q.data_ptr(),
         (const unsigned char*)z2q.data_ptr(), n1.data_ptr<float>(),
         n2.data_ptr<float>(), out.data_ptr<float>(), n, m, dp,
         (float)(amplitude * amplitude), (float)(scale * scale),
         current_stream());
  return out;
}

torch::Tensor posterior_scores_chunked(
    torch::Tensor xq, torch::Tensor x, torch::Tensor lengthscales,
    double amplitude, double mean_c, torch::Tensor alpha,
    torch::Tensor kinv, torch::Tensor onehot, int64_t acq, double coef,
    double best_value, double tr_radius) {
  xq = check_f32(xq, "xq");
  x = check_f32(x, "x");
  lengthscales = check_f32(lengthscales, "lengthscales");
  alpha = check_f32(alpha, "alpha");
  kinv = check_f32(kinv, "kinv");
  check_scorer_args(xq, x, lengthscales, alpha, kinv, onehot);
  onehot = onehot.contiguous();
  const int b = xq.size(0), d = xq.size(1), n = x.size(0);
  TORCH_CHECK(d <= 512, "posterior_scores supports D <= 512");
  auto inv_ls = 1.0f / lengthscales;
  const AcqArgs a{(float)(amplitude * amplitude), (float)mean_c, (int)acq,
                  (float)coef, (float)best_value, (float)tr_radius};
  const QuadRoute route = quad_route(n, b);
  ScorerWs ws(xq, n);
  if (route == QuadRoute::kLegacy) {
    // This binding's legacy path is one launcher for all three kernels:
    // ps_kvec, the NCHUNK quadform, ps_finalize.
    auto var_ws = torch::empty({b, kLegacyNchunk}, xq.options());
    auto out = torch::empty({b}, xq.options());
    launch_posterior_score_chunked(
        xq.data_ptr<float>(), x.data_ptr<float>(), inv_ls.data_ptr<float>(),
        alpha.data_ptr<float>(), kinv.data_ptr<float>(),
        onehot.data_ptr<unsigned char>(), ws.k.data_ptr<float>(),
        ws.mu.data_ptr<float>(), ws.dist.data_ptr<float>(),
        var_ws.data_ptr<float>(), out.data_ptr<float>(), b, n, d, a.amp2,
        a.mean_c, a.acq, a.coef, a.best_value, a.tr_radius,
        current_stream());
    return out;
  }
  // The fp32 bindings (this one and posterior_mean_std) switch to the
  // row-split k-vector on the GEMM route; bf16 and fp8 have one k-vector
  // kernel each for every N.
  kvec_f32(xq, x, inv_ls, alpha, onehot, ws, a.amp2,
           route == QuadRoute::kGemm);
  return finalize_score(ws, quadform(route, ws, kinv), a);
}

// -- Monte-Carlo qEI over candidate sets (qei_score.hip) ------------------

namespace {

constexpr int kQeiMaxParallel = 16;  // == eagle.HIP_MAX_PARALLEL

struct QeiJoint {
  torch::Tensor mean;     // (B, q)
  torch::Tensor cov;      // (B, q, q)
  torch::Tensor dist_ws;  // (B*q,) min L-inf distance of EVERY member
};

// Stages A-C: k-vectors of the B*q flattened candidates, T = k @ Kinv as
// one SGEMM (Kinv read once, as quadform_large_n does), then the joint
// mean / covariance kernel. No N-dependent branch: B*q workgroups already
// fill the chip, so the row-split k-vector kernel is never needed here.
// No host sync anywhere, so the sequence is stream-capturable.
QeiJoint qei_joint_impl(torch::Tensor xs, torch::Tensor x,
                        torch::Tensor lengthscales, double amplitude,
                        double mean_c, torch::Tensor alpha,
                        torch::Tensor kinv, torch::Tensor onehot) {
  xs = check_f32(xs, "xs");
  TORCH_CHECK(xs.dim() == 3, "xs must be (B, q, D), got ", xs.dim(),
              " dimensions");
  const int64_t b = xs.size(0), q = xs.size(1), d = xs.size(2);
  TORCH_CHECK(b >= 1, "xs must hold at least one candidate set");
  TORCH_CHECK(q >= 1 && q <= kQeiMaxParallel, "qEI set scorer supports ",
              "1 <= q <= ", kQeiMaxParallel, ", got q = ", q);
  TORCH_CHECK(d <= 512, "qEI set scorer supports D <= 512, got ", d);
  x = check_f32(x, "x");
  lengthscales = check_f32(lengthscales, "lengthscales");
  alpha = check_f32(alpha, "alpha");
  kinv = check_f32(kinv, "kinv");
  auto flat = xs.view({b * q, d});
  check_scorer_args(flat, x, lengthscales, alpha, kinv, onehot);
  onehot = onehot.contiguous();
  const int64_t n = x.size(0);
  TORCH_CHECK(b * q * std::max<int64_t>(n, q) < (int64_t{1} << 31),
              "qEI set scorer workspace too large");
  const float amp2 = (float)(amplitude * amplitude);
  auto inv_ls = 1.0f / lengthscales;
  auto k_ws = torch::empty({b * q, n}, xs.options());
  auto mu_ws = torch::empty({b * q}, xs.options());
  auto dist_ws = torch::empty({b * q}, xs.options());
  launch_ps_kvec(flat.data_ptr<float>(), x.data_ptr<float>(),
                 inv_ls.data_ptr<float>(), alpha.data_ptr<float>(),
                 onehot.data_ptr<unsigned char>(), k_ws.data_ptr<float>(),
                 mu_ws.data_ptr<float>(), dist_ws.data_ptr<float>(),
                 (int)(b * q), (int)n, (int)d, amp2, current_stream());
  auto t_ws = at::matmul(k_ws, kinv).contiguous();
  auto mean = torch::empty({b, q}, xs.options());
  auto cov = torch::empty({b, q, q}, xs.options());
  launch_qei_cov(t_ws.data_ptr<float>(), k_ws.data_ptr<float>(),
                 mu_ws.data_ptr<float>(), xs.data_ptr<float>(),
                 inv_ls.data_ptr<float>(), mean.data_ptr<float>(),
                 cov.data_ptr<float>(), (int)b, (int)q, (int)n, (int)d,
                 amp2, (float)mean_c, current_stream());
  return {mean, cov, dist_ws};
}

// Stage D. dist_ws: (B*q,) distances (member 0 of each set is read), or
// undefined for no trust region.
torch::Tensor qei_mc_impl(const torch::Tensor& mean,
                          const torch::Tensor& cov, torch::Tensor eps,
                          double best_value, const torch::Tensor& dist_ws,
                          double tr_radius) {
  const int64_t b = mean.size(0), q = mean.size(1);
  eps = check_f32(eps, "eps");
  TORCH_CHECK(eps.dim() == 2, "eps must be (S, q)");
  TORCH_CHECK(eps.size(1) == q, "eps must have q = ", q,
              " columns, got ", eps.size(1));
  const int64_t s = eps.size(0);
  TORCH_CHECK(s >= 1, "eps must hold at least one sample");
  TORCH_CHECK(s * q < (int64_t{1} << 31), "eps too large");
  auto out = torch::empty({b}, mean.options());
  launch_qei_mc(mean.data_ptr<float>(), cov.data_ptr<float>(),
                eps.data_ptr<float>(),
                dist_ws.defined() ? dist_ws.data_ptr<float>() : nullptr,
                out.data_ptr<float>(), (int)b, (int)q, (int)s,
                (float)best_value, (float)tr_radius, current_stream());
  return out;
}

}  // namespace

std::vector<torch::Tensor> qei_joint_mean_cov(
    torch::Tensor xs, torch::Tensor x, torch::Tensor lengthscales,
    double amplitude, double mean_c, torch::Tensor alpha,
    torch::Tensor kinv, torch::Tensor onehot) {
  auto j = qei_joint_impl(xs, x, lengthscales, amplitude, mean_c, alpha,
                          kinv, onehot);
  const int64_t b = j.mean.size(0), q = j.mean.size(1);
  return {j.mean, j.cov, j.dist_ws.view({b, q}).select(1, 0).contiguous()};
}

torch::Tensor qei_scores_from_cov(torch::Tensor mean, torch::Tensor cov,
                                  torch::Tensor eps, double best_value) {
  mean = check_f32(mean, "mean");
  cov = check_f32(cov, "cov");
  TORCH_CHECK(mean.dim() == 2, "mean must be (B, q)");
  const int64_t b = mean.size(0), q = mean.size(1);
  TORCH_CHECK(b >= 1, "mean must hold at least one candidate set");
  TORCH_CHECK(q >= 1 && q <= kQeiMaxParallel, "qEI set scorer supports ",
              "1 <= q <= ", kQeiMaxParallel, ", got q = ", q);
  TORCH_CHECK(cov.dim() == 3 && cov.size(0) == b && cov.size(1) == q &&
              cov.size(2) == q, "cov must be (", b, ", ", q, ", ", q, ")");
  return qei_mc_impl(mean, cov, eps, best_value, torch::Tensor(), 0.0);
}

torch::Tensor qei_set_scores(
    torch::Tensor xs, torch::Tensor x, torch::Tensor lengthscales,
    double amplitude, double mean_c, torch::Tensor alpha,
    torch::Tensor kinv, torch::Tensor onehot, torch::Tensor eps,
    double best_value, double tr_radius) {
  // Check eps before anything is launched.
  TORCH_CHECK(xs.dim() == 3 && eps.dim() == 2 &&
              eps.size(1) == xs.size(1),
              "eps must be (S, q) with q = xs.size(1)");
  auto j = qei_joint_impl(xs, x, lengthscales, amplitude, mean_c, alpha,
                          kinv, onehot);
  return qei_mc_impl(j.mean, j.cov, eps, best_value, j.dist_ws, tr_radius);
}

torch::Tensor posterior_scores_bf16(
    torch::Tensor xq, torch::Tensor x, torch::Tensor z2b,
    torch::Tensor n2, torch::Tensor lengthscales, double amplitude,
    double mean_c, torch::Tensor alpha, torch::Tensor kinv,
    torch::Tensor onehot, int64_t acq, double coef, double best_value,
    double tr_radius) {
  // bf16 candidate grams against CACHED training operands (z2b =
  // bf16(x / lengthscales), n2 = rounded row norms — computed once per
  // suggest by ScoringFunction). Same 3-launch graph-capturable shape
  // as the fp32 chunked scorer.
  xq = check_f32(xq, "xq");
  x = check_f32(x, "x");
  n2 = check_f32(n2, "n2");
  lengthscales = check_f32(lengthscales, "lengthscales");
  alpha = check_f32(alpha, "alpha");
  kinv = check_f32(kinv, "kinv");
  TORCH_CHECK(z2b.scalar_type() == torch::kBFloat16 && z2b.is_cuda(),
              "z2b must be bf16 cuda");
  check_scorer_args(xq, x, lengthscales, alpha, kinv, onehot);
  check_cached_operands(z2b, n2, x, "z2b");
  z2b = z2b.contiguous();
  onehot = onehot.contiguous();
  const int b = xq.size(0), d = xq.size(1), n = x.size(0);
  const int dp = z2b.size(1);
  TORCH_CHECK(dp % 32 == 0 && dp <= 512, "dp must be mult of 32, <=512");
  TORCH_CHECK(dp >= d, "z2b must have at least ", d, " columns");
  auto inv_ls = 1.0f / lengthscales;
  const AcqArgs a{(float)(amplitude * amplitude), (float)mean_c, (int)acq,
                  (float)coef, (float)best_value, (float)tr_radius};
  ScorerWs ws(xq, n);
  launch_ps_kvec_bf16(
      xq.data_ptr<float>(), x.data_ptr<float>(),
      (const unsigned short*)z2b.data_ptr(), n2.data_ptr<float>(),
      inv_ls.data_ptr<float>(), alpha.data_ptr<float>(),
      onehot.data_ptr<unsigned char>(), ws.k.data_ptr<float>(),
      ws.mu.data_ptr<float>(), ws.dist.data_ptr<float>(), b, n, d, dp,
      a.amp2, current_stream());
  const QuadRoute route = quad_route(n, b);
  if (route == QuadRoute::kLegacy) {
    // This binding's legacy path: one launcher for the NCHUNK quadform
    // and ps_finalize.
    auto var_ws = torch::empty({b, kLegacyNchunk}, xq.options());
    auto out = torch::empty({b}, xq.options());
    launch_ps_quadform_finalize(
        ws.k.data_ptr<float>(), kinv.data_ptr<float>(),
        ws.mu.data_ptr<float>(), ws.dist.data_ptr<float>(),
        var_ws.data_ptr<float>(), out.data_ptr<float>(), b, n, a.amp2,
        a.mean_c, a.acq, a.coef, a.best_value, a.tr_radius,
        current_stream());
    return out;
  }
  return finalize_score(ws, quadform(route, ws, kinv), a);
}

std::vector<torch::Tensor> posterior_mean_std(
    torch::Tensor xq, torch::Tensor x, torch::Tensor lengthscales,
    double amplitude, double mean_c, torch::Tensor alpha,
    torch::Tensor kinv, torch::Tensor onehot) {
  // (mean, sd, min-Linf dist) for one GP over a candidate batch in
  // 3-4 launches — the per-metric piece of the fused MO scorer.
  xq = check_f32(xq, "xq");
  x = check_f32(x, "x");
  lengthscales = check_f32(lengthscales, "lengthscales");
  alpha = check_f32(alpha, "alpha");
  kinv = check_f32(kinv, "kinv");
  check_scorer_args(xq, x, lengthscales, alpha, kinv, onehot);
  onehot = onehot.contiguous();
  const int b = xq.size(0), d = xq.size(1), n = x.size(0);
  TORCH_CHECK(d <= 512, "posterior_mean_std supports D <= 512");
  auto inv_ls = 1.0f / lengthscales;
  const float amp2 = (float)(amplitude * amplitude);
  const QuadRoute route = quad_route(n, b);
  ScorerWs ws(xq, n);
  kvec_f32(xq, x, inv_ls, alpha, onehot, ws, amp2,
           route == QuadRoute::kGemm);
  if (route == QuadRoute::kLegacy) {
    // This binding's legacy path: the NCHUNK quadform alone, then the
    // partial-sum form of the finalize.
    auto var_ws = torch::empty({b, kLegacyNchunk}, xq.options());
    launch_ps_quadform_kernel_only(
        ws.k.data_ptr<float>(), kinv.data_ptr<float>(),
        var_ws.data_ptr<float>(), b, n, current_stream());
    return finalize_meanstd(ws, var_ws, kLegacyNchunk, amp2,
                            (float)mean_c);
  }
  return finalize_meanstd(ws, quadform(route, ws, kinv), 0, amp2,
                          (float)mean_c);
}

std::vector<torch::Tensor> posterior_mean_std_fp8(
    torch::Tensor xq, torch::Tensor x, torch::Tensor z2q,
    torch::Tensor n2, double scale, torch::Tensor lengthscales,
    double amplitude, double mean_c, torch::Tensor alpha,
    torch::Tensor kinv, torch::Tensor onehot) {
  // (mean, sd, dist) with fp8 candidate grams against cached training
  // operands (Fp8GramCache layout) — the per-metric piece of the
  // fused MO fp8 scorer (config 5).
  xq = check_f32(xq, "xq");
  x = check_f32(x, "x");
  n2 = check_f32(n2, "n2");
  lengthscales = check_f32(lengthscales, "lengthscales");
  alpha = check_f32(alpha, "alpha");
  kinv = check_f32(kinv, "kinv");
  TORCH_CHECK(z2q.scalar_type() == torch::kFloat8_e4m3fn,
              "z2q must be float8_e4m3fn");
  check_scorer_args(xq, x, lengthscales, alpha, kinv, onehot);
  check_cached_operands(z2q, n2, x, "z2q");
  z2q = z2q.contiguous();
  onehot = onehot.contiguous();
  const int b = xq.size(0), d = xq.size(1), n = x.size(0);
  const int dp = z2q.size(1);
  TORCH_CHECK(dp % 32 == 0 && dp <= 512, "dp must be mult of 32, <=512");
  TORCH_CHECK(dp >= d, "z2q must have at least ", d, " columns");
  // Candidate side: quantize + dequantize with torch (tiny, no sync).
  auto z1 = xq / lengthscales;
  auto z1q = torch::zeros({b, dp},
                          xq.options().dtype(torch::kFloat8_e4m3fn));
  z1q.index_put_({torch::indexing::Slice(),
                  torch::indexing::Slice(0, d)},
                 (z1 / scale).to(torch::kFloat8_e4m3fn));
  auto z1f = z1q.to(torch::kFloat32) * scale;
  auto n1 = (z1f * z1f).sum(-1);
  const float amp2 = (float)(amplitude * amplitude);
  ScorerWs ws(xq, n);
  launch_ps_kvec_fp8(
      z1f.contiguous().data_ptr<float>(), n1.contiguous().data_ptr<float>(),
      xq.data_ptr<float>(), x.data_ptr<float>(),
      (const unsigned char*)z2q.data_ptr(), n2.data_ptr<float>(),
      alpha.data_ptr<float>(), onehot.data_ptr<unsigned char>(),
      ws.k.data_ptr<float>(), ws.mu.data_ptr<float>(),
      ws.dist.data_ptr<float>(), b, n, d, dp, amp2, (float)scale,
      current_stream());
  // This binding has no legacy NCHUNK path: below the threshold, b > 32
  // goes to the GEMM route where the other three take their legacy
  // kernels.
  const QuadRoute route = quad_route(n, b) == QuadRoute::kTile
      ? QuadRoute::kTile : QuadRoute::kGemm;
  return finalize_meanstd(ws, quadform(route, ws, kinv), 0, amp2,
                          (float)mean_c);
}

// -- Set-PE logdet scorer of GP-UCB-PE (setpe_score.hip) -------------------

namespace {

// The tail: one wave per set. mean / sd / dist hold one value per member
// of the flattened batch; dist undefined means no trust region.
torch::Tensor setpe_tail_impl(const torch::Tensor& cov,
                              const torch::Tensor& mean,
                              const torch::Tensor& sd,
                              const torch::Tensor& dist, double jitter,
                              double threshold, double explore_coef,
                              double penalty_coef, double tr_radius) {
  const int64_t b = cov.size(0), q = cov.size(1);
  auto out = torch::empty({b}, cov.options());
  launch_setpe_logdet(cov.data_ptr<float>(), mean.data_ptr<float>(),
                      sd.data_ptr<float>(),
                      dist.defined() ? dist.data_ptr<float>() : nullptr,
                      out.data_ptr<float>(), (int)b, (int)q, (float)jitter,
                      (float)threshold, (float)explore_coef,
                      (float)penalty_coef, (float)tr_radius,
                      current_stream());
  return out;
}

}  // namespace

torch::Tensor setpe_scores_from_cov(
    torch::Tensor cov, torch::Tensor mean, torch::Tensor sd,
    c10::optional<torch::Tensor> dist, double jitter, double threshold,
    double explore_coef, double penalty_coef, double tr_radius) {
  cov = check_f32(cov, "cov");
  mean = check_f32(mean, "mean");
  sd = check_f32(sd, "sd");
  TORCH_CHECK(cov.dim() == 3 && cov.size(1) == cov.size(2),
              "cov must be (B, q, q)");
  const int64_t b = cov.size(0), q = cov.size(1);
  TORCH_CHECK(b >= 1, "cov must hold at least one candidate set");
  TORCH_CHECK(q >= 1 && q <= kQeiMaxParallel, "set-PE scorer supports ",
              "1 <= q <= ", kQeiMaxParallel, ", got q = ", q);
  TORCH_CHECK(b * q * q < (int64_t{1} << 31), "cov too large");
  TORCH_CHECK(mean.numel() == b * q, "mean must have B q = ", b * q,
              " elements, got ", mean.numel());
  TORCH_CHECK(sd.numel() == b * q, "sd must have B q = ", b * q,
              " elements, got ", sd.numel());
  torch::Tensor dist_t;
  if (dist.has_value()) {
    dist_t = check_f32(*dist, "dist");
    TORCH_CHECK(dist_t.numel() == b * q, "dist must have B q = ", b * q,
                " elements, got ", dist_t.numel());
  }
  return setpe_tail_impl(cov, mean, sd, dist_t, jitter, threshold,
                         explore_coef, penalty_coef, tr_radius);
}

torch::Tensor setpe_set_scores(
    torch::Tensor xs, torch::Tensor post_x, torch::Tensor post_alpha,
    torch::Tensor post_kinv, double post_mean_c, torch::Tensor all_x,
    torch::Tensor all_kinv, torch::Tensor lengthscales, double amplitude,
    torch::Tensor onehot, double threshold, double explore_coef,
    double penalty_coef, double tr_radius) {
  // Every operand of BOTH posteriors is checked here, before the first
  // launch; the stages below repeat their own checks on the same values.
  xs = check_f32(xs, "xs");
  TORCH_CHECK(xs.dim() == 3, "xs must be (B, q, D), got ", xs.dim(),
              " dimensions");
  const int64_t b = xs.size(0), q = xs.size(1), d = xs.size(2);
  TORCH_CHECK(b >= 1, "xs must hold at least one candidate set");
  TORCH_CHECK(q >= 1 && q <= kQeiMaxParallel, "set-PE scorer supports ",
              "1 <= q <= ", kQeiMaxParallel, ", got q = ", q);
  TORCH_CHECK(d <= 512, "set-PE scorer supports D <= 512, got ", d);
  post_x = check_f32(post_x, "post_x");
  post_alpha = check_f32(post_alpha, "post_alpha");
  post_kinv = check_f32(post_kinv, "post_kinv");
  all_x = check_f32(all_x, "all_x");
  all_kinv = check_f32(all_kinv, "all_kinv");
  lengthscales = check_f32(lengthscales, "lengthscales");
  auto flat = xs.view({b * q, d});
  check_scorer_args(flat, post_x, lengthscales, post_alpha, post_kinv,
                    onehot);
  TORCH_CHECK(all_x.dim() == 2 && all_x.size(1) == d,
              "all_x must have xs's ", d, " columns");
  const int64_t n = post_x.size(0), n_all = all_x.size(0);
  TORCH_CHECK(all_kinv.dim() == 2 && all_kinv.size(0) == n_all &&
              all_kinv.size(1) == n_all, "all_kinv must be (", n_all, ", ",
              n_all, ")");
  TORCH_CHECK(b * q * std::max<int64_t>(std::max(n, n_all), q) <
              (int64_t{1} << 31), "set-PE scorer workspace too large");
  // (mean, sd) of every member under the completed-trials posterior.
  auto explore = posterior_mean_std(flat, post_x, lengthscales, amplitude,
                                    post_mean_c, post_alpha, post_kinv,
                                    onehot);
  // Joint covariance under the completed + pending posterior (only the
  // variance is used: alpha = 0), and every member's distance to all_x.
  auto j = qei_joint_impl(xs, all_x, lengthscales, amplitude, 0.0,
                          torch::zeros({n_all}, xs.options()), all_kinv,
                          onehot);
  return setpe_tail_impl(j.cov, explore[0], explore[1], j.dist_ws,
                         1e-10 * amplitude * amplitude, threshold,
                         explore_coef, penalty_coef, tr_radius);
}

torch::Tensor hv_scalarize_tr(
    torch::Tensor means, torch::Tensor sds, torch::Tensor weights,
    c10::optional<torch::Tensor> ref, c10::optional<torch::Tensor> dist,
    double coef, double tr_radius) {
  means = check_f32(means, "means");    // (M, B)
  sds = check_f32(sds, "sds");
  weights = check_f32(weights, "weights");  // (S, M)
  const int m = means.size(0), b = means.size(1);
  const int s = weights.size(0);
  TORCH_CHECK(weights.size(1) == m, "weights/means metric mismatch");
  TORCH_CHECK(sds.sizes() == means.sizes(),
              "sds must have the shape of means");
  torch::Tensor ref_t, dist_t;
  const float* ref_p = nullptr;
  const float* dist_p = nullptr;
  if (ref.has_value()) {
    ref_t = check_f32(*ref, "ref");
    TORCH_CHECK(ref_t.numel() == m, "ref must have ", m,
                " elements, got ", ref_t.numel());
    ref_p = ref_t.data_ptr<float>();
  }
  if (dist.has_value()) {
    dist_t = check_f32(*dist, "dist");
    TORCH_CHECK(dist_t.numel() == b, "dist must have ", b,
                " elements, got ", dist_t.numel());
    dist_p = dist_t.data_ptr<float>();
  }
  auto out = torch::empty({b}, means.options());
  launch_hv_scalarize_tr(
      means.data_ptr<float>(), sds.data_ptr<float>(),
      weights.data_ptr<float>(), ref_p, dist_p,
      out.data_ptr<float>(), b, m, s, (float)coef, (float)tr_radius,
      current_stream());
  return out;
}

// `impl` is "v2" or "v6"; "" means VIZIER_AMD_CHOL_IMPL, read once per
// process, and v6 when that is unset or names neither. v2 and v6 factor
// the same bits (tests/test_potrf_tiled.py). Timings at N = 1000:
//   v6 (default): v2's two launches per 32-column round, trailing update
//       on 64 x 64 tiles and a column-wise panel solve: 0.53 / 0.63 /
//       0.71 ms at R = 2 / 8 / 16 (profiles/bench_potrf_tiled.md).
//   v2: 2.8 ms whatever R. A 63-deep chain of trivial kernels runs at
//       4.4 us per launch and LDS-staged coalescing changed nothing, so
//       the ~45 us per kernel were taken for an end-of-kernel fence. They
//       are the serial chain inside the critical workgroup: one strip's
//       workgroup walks every row below it, and each panel row is a
//       528-step dependent chain. v6 runs the same rounds with the same
//       kernel boundaries in under a quarter of the time.
// DESIGN.md describes the retired designs (v1, v3, v4, v5) and what they
// measured.
int resolve_potrf_impl(const std::string& impl) {
  const auto parse = [](const std::string& s) {
    return s == "v2" ? 2 : s == "v6" ? 6 : 0;
  };
  if (!impl.empty()) {
    const int version = parse(impl);
    TORCH_CHECK(version != 0, "batched_potrf impl must be one of v2, v6, "
                "got '", impl, "'");
    return version;
  }
  static const int from_env = [&]() {
    const char* env = std::getenv("VIZIER_AMD_CHOL_IMPL");
    const int version = parse(env == nullptr ? "" : env);
    return version != 0 ? version : 6;
  }();
  return from_env;
}

// What the v2 / v6 launcher runs for an n x n matrix: (rows per panel
// workgroup, panel row tiles of round 0, trailing workgroups per matrix
// of round 0, 1 if it parks diagonal blocks in a scratch tensor else 0).
// Round 0 is the largest round. Pure host arithmetic.
std::vector<int64_t> batched_potrf_launch_shape_py(int64_t n,
                                                   const std::string& impl) {
  const int version = resolve_potrf_impl(impl);
  TORCH_CHECK(n >= 1, "n must be >= 1");
  int out[2];
  batched_potrf_launch_shape((int)n, version, out);
  return {batched_potrf_panel_rows(version), out[0], out[1],
          batched_potrf_needs_scratch((int)n, version)};
}

std::vector<torch::Tensor> batched_potrf(torch::Tensor K,
                                         const std::string& impl_name) {
  // (R, N, N) -> (L in a fresh tensor, info (R,) int32). Only the LOWER
  // triangle of L is defined: the default path leaves K's values in the
  // strict upper triangle outside the 32x32 diagonal blocks, and
  // batched_trsv_lower never reads it. info[r] is the 1-based first
  // column whose pivot is not > 0 (zero, negative or NaN), else 0.
  K = check_f32(K, "K");
  TORCH_CHECK(K.dim() == 3 && K.size(1) == K.size(2),
              "K must be (R, N, N)");
  TORCH_CHECK(K.size(0) >= 1 && K.size(1) >= 1,
              "batched_potrf needs R >= 1 and N >= 1, got R = ",
              K.size(0), ", N = ", K.size(1));
  const int r = K.size(0), n = K.size(1);
  const int impl = resolve_potrf_impl(impl_name);
  auto info = torch::zeros({r}, K.options().dtype(torch::kInt32));
  auto L = K.clone();
  // Rounds with more than one row tile park their factored diagonal
  // block here instead of overwriting what the other tiles still read.
  torch::Tensor dscratch;
  float* dscratch_p = nullptr;
  if (batched_potrf_needs_scratch(n, impl)) {
    dscratch = torch::empty({r, 32, 32}, K.options());
    dscratch_p = dscratch.data_ptr<float>();
  }
  launch_batched_potrf(L.data_ptr<float>(), info.data_ptr<int>(),
                       dscratch_p, r, n, impl, current_stream());
  return {L, info};
}

// variant 0: the pipelined register-resident solve (N <= 1280; larger N
// runs variant 1). variant 1: the LDS-staged solve. Same bits either way.
torch::Tensor batched_trsv_lower(torch::Tensor L, torch::Tensor b,
                                 int64_t variant) {
  TORCH_CHECK(variant == 0 || variant == 1,
              "batched_trsv_lower variant must be 0 or 1, got ", variant);
  L = check_f32(L, "L");
  b = check_f32(b, "b");
  TORCH_CHECK(L.dim() == 3 && L.size(1) == L.size(2) &&
              b.dim() == 2 && b.size(0) == L.size(0) &&
              b.size(1) == L.size(1), "shape mismatch");
  TORCH_CHECK(L.size(0) >= 1 && L.size(1) >= 1,
              "batched_trsv_lower needs R >= 1 and N >= 1, got R = ",
              L.size(0), ", N = ", L.size(1));
  auto z = b.clone();
  launch_batched_trsv_lower(L.data_ptr<float>(), z.data_ptr<float>(),
                            (int)L.size(0), (int)L.size(1), (int)variant,
                            current_stream());
  return z;
}

// -- Eagle step bindings ------------------------------------------------------
//
// The fp32 and fp64 kernels are instantiations of one template
// (eagle_step.hip), so the two pairs of bindings share their argument
// checks and their bodies. Every check throws before anything is launched.

torch::Tensor check_f64(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == torch::kFloat64, name, " must be fp64");
  return t.contiguous();
}

torch::Tensor check_real(const torch::Tensor& t, torch::ScalarType dtype,
                         const char* name) {
  return dtype == torch::kFloat64 ? check_f64(t, name) : check_f32(t, name);
}

// Tensors the Eagle kernels update in place: never copied.
void check_inplace(const torch::Tensor& t, torch::ScalarType dtype,
                   const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == dtype &&
              t.is_contiguous(), name,
              " must be a contiguous GPU tensor of the kernel's dtype");
}

struct EagleShape {
  int pool_size, batch_size, q, dc, dcat;
};

// Read-only operands are replaced by contiguous images; out_cont, out_cat
// and iter_counter are written in place.
EagleShape check_eagle_suggest_args(
    torch::Tensor& pool_cont, torch::Tensor& pool_cat,
    torch::Tensor& rewards, torch::Tensor& perturbations,
    torch::Tensor& cat_sizes, const torch::Tensor& iter_counter,
    int64_t n_batches, int64_t batch_size, const torch::Tensor& out_cont,
    const torch::Tensor& out_cat, int64_t max_cat,
    torch::ScalarType dtype) {
  pool_cont = check_real(pool_cont, dtype, "pool_cont");
  rewards = check_real(rewards, dtype, "rewards");
  perturbations = check_real(perturbations, dtype, "perturbations");
  TORCH_CHECK(iter_counter.scalar_type() == torch::kInt64 &&
              iter_counter.is_cuda() && iter_counter.is_contiguous() &&
              iter_counter.numel() >= 2,
              "iter_counter must be int64 cuda with >= 2 slots");
  TORCH_CHECK(pool_cont.dim() == 3 && pool_cat.dim() == 3,
              "pool_cont / pool_cat must be (P, q, D*)");
  TORCH_CHECK(pool_cat.is_cuda() &&
              pool_cat.scalar_type() == torch::kInt64 &&
              cat_sizes.is_cuda() &&
              cat_sizes.scalar_type() == torch::kInt64,
              "pool_cat / cat_sizes must be int64 GPU tensors");
  pool_cat = pool_cat.contiguous();
  cat_sizes = cat_sizes.contiguous();
  EagleShape s;
  s.pool_size = pool_cont.size(0);
  s.batch_size = (int)batch_size;
  s.q = pool_cont.size(1);
  s.dc = pool_cont.size(2);
  s.dcat = pool_cat.size(2);
  // The kernel keeps scale[MAX_POOL = 128] in LDS, normalises noise
  // over q <= MAX_Q = 16, and indexes the pool by batch_start + b <
  // n_batches * batch_size.
  TORCH_CHECK(pool_cont.size(0) >= 1 && pool_cont.size(0) <= 128,
              "the Eagle step kernels support 1 <= pool <= 128, got ",
              pool_cont.size(0));
  TORCH_CHECK(s.q >= 1 && s.q <= 16,
              "the Eagle step kernels support 1 <= q <= 16, got ", s.q);
  TORCH_CHECK(batch_size >= 1 && n_batches >= 1 &&
              n_batches * batch_size <= s.pool_size,
              "n_batches * batch_size must not exceed the pool");
  TORCH_CHECK(pool_cat.size(0) == s.pool_size && pool_cat.size(1) == s.q &&
              rewards.numel() == s.pool_size &&
              perturbations.numel() == s.pool_size &&
              cat_sizes.numel() == s.dcat, "pool shape mismatch");
  check_inplace(out_cont, dtype, "out_cont");
  check_inplace(out_cat, torch::kInt64, "out_cat");
  TORCH_CHECK(out_cont.numel() == batch_size * s.q * s.dc &&
              out_cat.numel() == batch_size * s.q * s.dcat,
              "out_cont / out_cat must be (batch, q, D*)");
  TORCH_CHECK(s.dcat == 0 || max_cat >= 1, "max_cat must be >= 1");
  return s;
}

// The pool, rewards, perturbations, best_reward and iter_counter are
// updated in place; the batch operands are replaced by contiguous images.
EagleShape check_eagle_update_args(
    const torch::Tensor& pool_cont, const torch::Tensor& pool_cat,
    const torch::Tensor& rewards, const torch::Tensor& perturbations,
    torch::Tensor& batch_cont, torch::Tensor& batch_cat,
    torch::Tensor& batch_rewards, torch::Tensor& cat_sizes,
    const torch::Tensor& best_reward, const torch::Tensor& iter_counter,
    int64_t n_batches, torch::ScalarType dtype) {
  check_inplace(pool_cont, dtype, "pool_cont");
  check_inplace(pool_cat, torch::kInt64, "pool_cat");
  check_inplace(rewards, dtype, "rewards");
  check_inplace(perturbations, dtype, "perturbations");
  check_inplace(best_reward, dtype, "best_reward");
  check_inplace(iter_counter, torch::kInt64, "iter_counter");
  batch_cont = check_real(batch_cont, dtype, "batch_cont");
  batch_rewards = check_real(batch_rewards, dtype, "batch_rewards");
  TORCH_CHECK(batch_cat.is_cuda() &&
              batch_cat.scalar_type() == torch::kInt64 &&
              cat_sizes.is_cuda() &&
              cat_sizes.scalar_type() == torch::kInt64,
              "batch_cat / cat_sizes must be int64 GPU tensors");
  batch_cat = batch_cat.contiguous();
  cat_sizes = cat_sizes.contiguous();
  TORCH_CHECK(pool_cont.dim() == 3 && pool_cat.dim() == 3 &&
              batch_cont.dim() == 3 && batch_cat.dim() == 3,
              "pool / batch tensors must be (rows, q, D*)");
  EagleShape s;
  s.pool_size = pool_cont.size(0);
  s.batch_size = batch_cont.size(0);
  s.q = batch_cont.size(1);
  s.dc = batch_cont.size(2);
  s.dcat = batch_cat.size(2);
  TORCH_CHECK(pool_cont.size(0) >= 1 && pool_cont.size(0) <= 128,
              "the Eagle step kernels support 1 <= pool <= 128, got ",
              pool_cont.size(0));
  TORCH_CHECK(s.q >= 1 && s.q <= 16,
              "the Eagle step kernels support 1 <= q <= 16, got ", s.q);
  TORCH_CHECK(s.batch_size >= 1 && n_batches >= 1 &&
              n_batches * s.batch_size <= s.pool_size,
              "n_batches * batch_size must not exceed the pool");
  TORCH_CHECK(pool_cont.size(1) == s.q && pool_cont.size(2) == s.dc &&
              pool_cat.size(0) == s.pool_size && pool_cat.size(1) == s.q &&
              pool_cat.size(2) == s.dcat &&
              batch_cat.size(0) == s.batch_size &&
              batch_cat.size(1) == s.q && rewards.numel() == s.pool_size &&
              perturbations.numel() == s.pool_size &&
              batch_rewards.numel() == s.batch_size &&
              cat_sizes.numel() == s.dcat && best_reward.numel() >= 1 &&
              iter_counter.numel() >= 2, "pool / batch shape mismatch");
  return s;
}

// One body per step for both precisions. Launch is the extern "C" launcher
// of the kernel's instantiation for T; the double arguments are narrowed
// to T here.
template <typename T, auto Launch>
std::vector<torch::Tensor> eagle_suggest_impl(
    torch::Tensor pool_cont, torch::Tensor pool_cat, torch::Tensor rewards,
    torch::Tensor perturbations, torch::Tensor cat_sizes,
    torch::Tensor iter_counter, int64_t n_batches, int64_t batch_size,
    double visibility, double gravity, double neg_gravity,
    double norm_scale, double cat_factor, double p_same, int64_t seed,
    torch::Tensor out_cont, torch::Tensor out_cat, int64_t max_cat) {
  const EagleShape s = check_eagle_suggest_args(
      pool_cont, pool_cat, rewards, perturbations, cat_sizes, iter_counter,
      n_batches, batch_size, out_cont, out_cat, max_cat,
      c10::CppTypeToScalarType<T>::value);
  Launch(
      pool_cont.data_ptr<T>(),
      s.dcat ? pool_cat.data_ptr<long>() : nullptr,
      rewards.data_ptr<T>(), perturbations.data_ptr<T>(),
      s.dcat ? cat_sizes.data_ptr<long>() : nullptr,
      out_cont.data_ptr<T>(),
      s.dcat ? out_cat.data_ptr<long>() : nullptr,
      (const unsigned long long*)iter_counter.data_ptr<int64_t>(),
      (int)n_batches, s.batch_size, s.pool_size, s.q, s.dc, s.dcat,
      (int)max_cat, (T)visibility, (T)gravity, (T)neg_gravity,
      (T)norm_scale, (T)cat_factor, (T)p_same, (unsigned long long)seed,
      current_stream());
  return {out_cont, out_cat};
}

template <typename T, auto Launch>
void eagle_update_impl(
    torch::Tensor pool_cont, torch::Tensor pool_cat, torch::Tensor rewards,
    torch::Tensor perturbations, torch::Tensor batch_cont,
    torch::Tensor batch_cat, torch::Tensor batch_rewards,
    torch::Tensor cat_sizes, torch::Tensor best_reward,
    torch::Tensor iter_counter, int64_t n_batches, double penalize_factor,
    double perturbation_lower_bound, double base_perturbation,
    int64_t seed) {
  const EagleShape s = check_eagle_update_args(
      pool_cont, pool_cat, rewards, perturbations, batch_cont, batch_cat,
      batch_rewards, cat_sizes, best_reward, iter_counter, n_batches,
      c10::CppTypeToScalarType<T>::value);
  Launch(
      pool_cont.data_ptr<T>(),
      s.dcat ? pool_cat.data_ptr<long>() : nullptr,
      rewards.data_ptr<T>(), perturbations.data_ptr<T>(),
      batch_cont.data_ptr<T>(),
      s.dcat ? batch_cat.data_ptr<long>() : nullptr,
      batch_rewards.data_ptr<T>(),
      s.dcat ? cat_sizes.data_ptr<long>() : nullptr,
      best_reward.data_ptr<T>(),
      (unsigned long long*)iter_counter.data_ptr<int64_t>(),
      (int)n_batches, s.batch_size, s.q, s.dc, s.dcat, (T)penalize_factor,
      (T)perturbation_lower_bound, (T)base_perturbation,
      (unsigned long long)seed, current_stream());
}

constexpr auto eagle_suggest =
    &eagle_suggest_impl<float, launch_eagle_suggest>;
constexpr auto eagle_suggest_f64 =
    &eagle_suggest_impl<double, launch_eagle_suggest_f64>;
constexpr auto eagle_update = &eagle_update_impl<float, launch_eagle_update>;
constexpr auto eagle_update_f64 =
    &eagle_update_impl<double, launch_eagle_update_f64>;

int64_t eagle_sweep(
    torch::Tensor pool_cont, torch::Tensor rewards,
    torch::Tensor perturbations, torch::Tensor best_reward,
    torch::Tensor iter_counter, torch::Tensor barrier_buf,
    torch::Tensor x, torch::Tensor inv_ls,
    torch::Tensor alpha, torch::Tensor kinv, torch::Tensor out_cont,
    torch::Tensor k_ws, torch::Tensor mu_ws, torch::Tensor dist_ws,
    torch::Tensor var_ws, int64_t n_batches,
    int64_t batch_size, int64_t pool_size, int64_t it_start,
    int64_t iterations, double visibility, double gravity,
    double neg_gravity, double norm_scale, double penalize_factor,
    double perturbation_lower_bound, double base_perturbation,
    int64_t seed_suggest, int64_t seed_update, double amp2,
    double mean_c, int64_t acq, double coef, double best_value,
    double tr_radius) {
  // Every check throws before anything is launched. The state and the
  // workspaces are written in place, so they are never copied: a
  // contiguous image would take the update and the caller's tensor none.
  check_inplace(pool_cont, torch::kFloat32, "pool_cont");
  check_inplace(rewards, torch::kFloat32, "rewards");
  check_inplace(perturbations, torch::kFloat32, "perturbations");
  check_inplace(best_reward, torch::kFloat32, "best_reward");
  check_inplace(iter_counter, torch::kInt64, "iter_counter");
  check_inplace(barrier_buf, torch::kInt32, "barrier_buf");
  check_inplace(out_cont, torch::kFloat32, "out_cont");
  check_inplace(k_ws, torch::kFloat32, "k_ws");
  check_inplace(mu_ws, torch::kFloat32, "mu_ws");
  check_inplace(dist_ws, torch::kFloat32, "dist_ws");
  check_inplace(var_ws, torch::kFloat32, "var_ws");
  x = check_f32(x, "x");
  inv_ls = check_f32(inv_ls, "inv_ls");
  alpha = check_f32(alpha, "alpha");
  kinv = check_f32(kinv, "kinv");
  // Word 0 counts barrier arrivals upwards over one launch: the caller
  // zeroes it before every call. Word 1 is unused.
  TORCH_CHECK(barrier_buf.numel() >= 2, "barrier_buf must be int32 (2,)");
  TORCH_CHECK(x.dim() == 2, "x must be (N, Dc)");
  const int64_t dc64 = x.size(1), n64 = x.size(0);
  // xq_lds[512] in the kernel is indexed by j < dc.
  TORCH_CHECK(dc64 >= 1 && dc64 <= 512,
              "eagle_sweep supports 1 <= Dc <= 512, got ", dc64);
  TORCH_CHECK(n64 >= 1 && n64 <= 8192,
              "eagle_sweep supports 1 <= N <= 8192, got ", n64);
  TORCH_CHECK(pool_size >= 1 && pool_size <= 128,
              "eagle_sweep supports 1 <= pool <= 128, got ", pool_size);
  TORCH_CHECK(batch_size >= 1 && batch_size <= 32,
              "eagle_sweep tile quadform supports 1 <= batch <= 32, got ",
              batch_size);
  TORCH_CHECK(n_batches >= 1 && n_batches * batch_size == pool_size,
              "pool_size must be n_batches * batch_size, got ", pool_size,
              " != ", n_batches, " * ", batch_size);
  TORCH_CHECK(iterations >= 0, "iterations must be >= 0, got ", iterations);
  const int dc = (int)dc64;
  const int n = (int)n64;
  TORCH_CHECK(pool_cont.numel() == pool_size * dc,
              "pool/feature shape mismatch (continuous-only, q=1)");
  TORCH_CHECK(rewards.numel() == pool_size &&
              perturbations.numel() == pool_size,
              "rewards / perturbations must have pool_size = ", pool_size,
              " elements");
  TORCH_CHECK(best_reward.numel() >= 1, "best_reward must not be empty");
  // [0:2] iteration counters, [2:12] the per-phase cycle accumulators.
  TORCH_CHECK(iter_counter.numel() >= 12,
              "iter_counter must have >= 12 slots, got ",
              iter_counter.numel());
  TORCH_CHECK(inv_ls.numel() == dc, "inv_ls must have ", dc,
              " elements, got ", inv_ls.numel());
  TORCH_CHECK(alpha.numel() == n, "alpha must have ", n, " elements, got ",
              alpha.numel());
  TORCH_CHECK(kinv.dim() == 2 && kinv.size(0) == n && kinv.size(1) == n,
              "kinv must be (", n, ", ", n, ")");
  TORCH_CHECK(out_cont.numel() >= batch_size * dc,
              "out_cont must hold batch * Dc elements");
  TORCH_CHECK(k_ws.numel() >= batch_size * n,
              "k_ws must hold batch * N elements");
  TORCH_CHECK(mu_ws.numel() >= batch_size && dist_ws.numel() >= batch_size,
              "mu_ws / dist_ws must hold batch elements");
  const long tiles_n = (n + 63) / 64;
  TORCH_CHECK(var_ws.numel() >= batch_size * (tiles_n * tiles_n + 1),
              "var_ws must be (B, tiles^2 + 1)");
  // Two parity slots of (candidates, mu, dist): phase A of iteration `it`
  // writes slot it & 1 and every owning workgroup reads it back in RC, so
  // the next iteration's A (which follows RC with no grid barrier) never
  // overwrites what a slower workgroup still reads. See eagle_sweep.hip.
  torch::Tensor slot_ws = torch::empty(
      {2, batch_size * (dc64 + 2)},
      torch::TensorOptions().dtype(torch::kFloat32).device(x.device()));
  const int ret = launch_eagle_sweep(
      pool_cont.data_ptr<float>(), rewards.data_ptr<float>(),
      perturbations.data_ptr<float>(), best_reward.data_ptr<float>(),
      (unsigned long long*)iter_counter.data_ptr<int64_t>(),
      (unsigned int*)barrier_buf.data_ptr<int>(),
      x.data_ptr<float>(), inv_ls.data_ptr<float>(),
      alpha.data_ptr<float>(), kinv.data_ptr<float>(),
      out_cont.data_ptr<float>(), k_ws.data_ptr<float>(),
      mu_ws.data_ptr<float>(), dist_ws.data_ptr<float>(),
      var_ws.data_ptr<float>(), slot_ws.data_ptr<float>(),
      (int)n_batches, (int)batch_size, (int)pool_size, dc, n,
      (long long)it_start, (long long)iterations, (float)visibility,
      (float)gravity, (float)neg_gravity, (float)norm_scale,
      (float)penalize_factor, (float)perturbation_lower_bound,
      (float)base_perturbation, (unsigned long long)seed_suggest,
      (unsigned long long)seed_update, (float)amp2, (float)mean_c,
      (int)acq, (float)coef, (float)best_value, (float)tr_radius,
      current_stream());
  TORCH_CHECK(ret > 0, "cooperative eagle_sweep launch failed (code ",
              ret, ")");
  return ret;
}

// -- fp64 parity-mode bindings -------------------------------------------------

// Runs the three fp64 scorer kernels on the current stream. `want_score`
// selects the (B,) acquisition score; otherwise mean and sd are written.
// Returns {score} or {mean, sd, dist}. No host sync: capturable.
std::vector<torch::Tensor> posterior_f64_impl(
    torch::Tensor xq, torch::Tensor x, torch::Tensor lengthscales,
    double amplitude, double mean_c, torch::Tensor alpha,
    torch::Tensor kinv, torch::Tensor onehot, bool want_score, int64_t acq,
    double coef, double best_value, double tr_radius) {
  xq = check_f64(xq, "xq");
  x = check_f64(x, "x");
  lengthscales = check_f64(lengthscales, "lengthscales");
  alpha = check_f64(alpha, "alpha");
  kinv = check_f64(kinv, "kinv");
  check_scorer_args(xq, x, lengthscales, alpha, kinv, onehot);
  onehot = onehot.contiguous();
  const int b = xq.size(0), d = xq.size(1), n = x.size(0);
  TORCH_CHECK(d <= 512, "posterior_scores_f64 supports D <= 512");
  TORCH_CHECK(b >= 1 && n >= 1, "posterior_scores_f64 needs B, N >= 1");
  TORCH_CHECK(acq >= 0 && acq <= 5, "unknown acquisition code ", acq);
  auto inv_ls = lengthscales.reciprocal();
  int ctiles = 0, slabs = 0, slab_rows = 0;
  ps_f64_quadform_shape(n, &ctiles, &slabs, &slab_rows);
  auto k_ws = torch::empty({b, n}, xq.options());
  auto mu_ws = torch::empty({b}, xq.options());
  auto dist_ws = torch::empty({b}, xq.options());
  auto part = torch::empty({b, (int64_t)ctiles * slabs}, xq.options());
  torch::Tensor out, mean, sd;
  double* out_p = nullptr;
  double* mean_p = nullptr;
  double* sd_p = nullptr;
  if (want_score) {
    out = torch::empty({b}, xq.options());
    out_p = out.data_ptr<double>();
  } else {
    mean = torch::empty({b}, xq.options());
    sd = torch::empty({b}, xq.options());
    mean_p = mean.data_ptr<double>();
    sd_p = sd.data_ptr<double>();
  }
  launch_posterior_score_f64(
      xq.data_ptr<double>(), x.data_ptr<double>(),
      inv_ls.data_ptr<double>(), alpha.data_ptr<double>(),
      kinv.data_ptr<double>(), onehot.data_ptr<unsigned char>(),
      k_ws.data_ptr<double>(), mu_ws.data_ptr<double>(),
      dist_ws.data_ptr<double>(), part.data_ptr<double>(), out_p, mean_p,
      sd_p, b, n, d, amplitude * amplitude, mean_c, (int)acq, coef,
      best_value, tr_radius, current_stream());
  if (want_score) return {out};
  return {mean, sd, dist_ws};
}

torch::Tensor posterior_scores_f64(
    torch::Tensor xq, torch::Tensor x, torch::Tensor lengthscales,
    double amplitude, double mean_c, torch::Tensor alpha,
    torch::Tensor kinv, torch::Tensor onehot, int64_t acq, double coef,
    double best_value, double tr_radius) {
  return posterior_f64_impl(xq, x, lengthscales, amplitude, mean_c, alpha,
                            kinv, onehot, true, acq, coef, best_value,
                            tr_radius)[0];
}

std::vector<torch::Tensor> posterior_mean_std_f64(
    torch::Tensor xq, torch::Tensor x, torch::Tensor lengthscales,
    double amplitude, double mean_c, torch::Tensor alpha,
    torch::Tensor kinv, torch::Tensor onehot) {
  return posterior_f64_impl(xq, x, lengthscales, amplitude, mean_c, alpha,
                            kinv, onehot, false, 4, 0.0, 0.0, 0.0);
}

torch::Tensor gram_matern52_f64(torch::Tensor x1, torch::Tensor x2,
                                torch::Tensor lengthscales,
                                double amplitude) {
  x1 = check_f64(x1, "x1");
  x2 = check_f64(x2, "x2");
  lengthscales = check_f64(lengthscales, "lengthscales");
  TORCH_CHECK(x1.dim() == 2 && x2.dim() == 2, "x1 and x2 must be 2-D");
  const int n = x1.size(0), m = x2.size(0), d = x1.size(1);
  TORCH_CHECK(x2.size(1) == d && lengthscales.numel() == d,
              "dimension mismatch");
  auto out = torch::empty({n, m}, x1.options());
  if (n == 0 || m == 0) return out;
  auto inv_ls = lengthscales.reciprocal();
  const int sym = (x1.data_ptr() == x2.data_ptr() && n == m) ? 1 : 0;
  launch_gram_matern52_f64(x1.data_ptr<double>(), x2.data_ptr<double>(),
                           inv_ls.data_ptr<double>(),
                           out.data_ptr<double>(), n, m, d,
                           amplitude * amplitude, sym, current_stream());
  return out;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("posterior_scores_f64", &posterior_scores_f64,
        "fp64 fused GP posterior scorer, MFMA f64 quadform (gfx950)");
  m.def("posterior_mean_std_f64", &posterior_mean_std_f64,
        "fp64 fused (mean, sd, dist) over candidates (gfx950)");
  m.def("gram_matern52_f64", &gram_matern52_f64,
        "fp64 difference-form Matern-5/2 Gram / cross-Gram (gfx950)");
  m.def("eagle_suggest_f64", eagle_suggest_f64,
        "fp64 fused Eagle suggest step (gfx950)");
  m.def("eagle_update_f64", eagle_update_f64,
        "fp64 fused Eagle update step (gfx950)");
  m.def("gram_matern52_batched", &gram_matern52_batched,
        "Batched-restart fused Matern-5/2 gram (+noise*I, optional "
        "gradient factor)");
  m.def("gram_matern52", &gram_matern52,
        "Fused Matern-5/2 ARD Gram matrix (gfx950)");
  m.def("gram_matern52_bf16", &gram_matern52_bf16,
        "bf16 MFMA Matern-5/2 Gram matrix (gfx950 matrix cores)");
  m.def("gram_matern52_bf16_tiled", &gram_matern52_bf16_tiled,
        "128x128 LDS-tiled bf16 MFMA Matern-5/2 Gram (gfx950)");
  m.def("gram_matern52_fp8", &gram_matern52_fp8,
        "fp8 e4m3 MFMA Matern-5/2 Gram matrix (gfx950, config 5)");
  m.def("gram_matern52_fp8_tiled", &gram_matern52_fp8_tiled,
        "128x128 LDS-tiled fp8 e4m3 MFMA Matern-5/2 Gram (gfx950)");
  m.def("posterior_scores", &posterior_scores,
        "Fused GP posterior + acquisition + trust region (gfx950)");
  m.def("batched_potrf", &batched_potrf,
        "Batched Cholesky K (R, N, N) fp32 -> (L, info). Only the lower "
        "triangle of L is defined; the strict upper triangle holds "
        "unspecified values. info[r] is the 1-based first column whose "
        "pivot is not > 0 (zero, negative or NaN), 0 on success. impl = "
        "v2 | v6; '' = VIZIER_AMD_CHOL_IMPL, else v6 (gfx950)",
        py::arg("K"), py::arg("impl") = "");
  m.def("batched_potrf_launch_shape", &batched_potrf_launch_shape_py,
        "(rows per panel workgroup, panel row tiles of round 0, trailing "
        "workgroups per matrix of round 0, uses scratch) of the v2 / v6 "
        "launcher for an n x n matrix; host arithmetic only",
        py::arg("n"), py::arg("impl") = "");
  m.def("batched_trsv_lower", &batched_trsv_lower,
        "Batched forward substitution L z = b (gfx950). variant 0 = "
        "pipelined register-resident solve, 1 = LDS-staged solve; "
        "bit-identical results",
        py::arg("L"), py::arg("b"), py::arg("variant") = 0);
  m.def("gram_matern52_fp8_pre", &gram_matern52_fp8_pre,
        "fp8 cross-gram from pre-quantized operands (gfx950)");
  m.def("posterior_mean_std_fp8", &posterior_mean_std_fp8,
        "Fused (mean, sd, dist) with fp8 cached-operand grams");
  m.def("posterior_mean_std", &posterior_mean_std,
        "Fused (mean, sd, dist) for one GP over candidates (gfx950)");
  m.def("hv_scalarize_tr", &hv_scalarize_tr,
        "Hypervolume scalarization + trust region in one launch");
  m.def("posterior_scores_bf16", &posterior_scores_bf16,
        "Chunked scorer with cached-bf16 candidate grams (gfx950)");
  m.def("posterior_scores_chunked", &posterior_scores_chunked,
        "3-kernel chunked GP posterior scorer (chip-filling, gfx950)");
  m.def("qei_joint_mean_cov", &qei_joint_mean_cov,
        "Joint posterior (mean, cov, member-0 dist) of candidate sets "
        "xs (B, q <= 16, D); assumes a symmetric kinv (gfx950)");
  m.def("qei_scores_from_cov", &qei_scores_from_cov,
        "Monte-Carlo qEI of (mean, cov) sets: q x q Cholesky with the "
        "diagonal fallback + max-improvement, no trust region (gfx950)");
  m.def("qei_set_scores", &qei_set_scores,
        "Fused Monte-Carlo qEI set scorer + trust region by member 0, "
        "stream-capturable (gfx950)");
  m.def("setpe_scores_from_cov", &setpe_scores_from_cov,
        "Set-PE tail: logdet of (cov + jitter I) by a one-wave Cholesky, "
        "-inf when not positive definite, + promising-region penalty + "
        "per-member trust region (gfx950)");
  m.def("setpe_set_scores", &setpe_set_scores,
        "Fused GP-UCB-PE set-PE scorer: explore (mean, sd), joint "
        "covariance under the completed + pending posterior, logdet tail; "
        "stream-capturable (gfx950)");
  m.def("eagle_suggest", eagle_suggest,
        "Fused Eagle suggest step (gfx950)");
  m.def("eagle_update", eagle_update, "Fused Eagle update step (gfx950)");
  m.def("eagle_sweep", &eagle_sweep,
        "Persistent cooperative Eagle sweep megakernel (gfx950)");
}
