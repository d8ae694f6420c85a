// Python bindings for the flowhip gfx950 HIP kernels (flowhip._C).

#include <torch/extension.h>

#include <cstdlib>
#include <vector>

#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAGuard.h>
#include <hip/hip_runtime.h>

// the conv family's geometry, plan and launchers
#include "conv_gemm.h"
#include "conv_fold.h"
// the normalized-convolution family's
#include "nconv.h"

// launchers defined in the other .hip translation units
void flowhip_bgemm_nt_launch(const void* A, const void* B, void* C,
                             float alpha, int batch, int M, int N, int K,
                             int out_bf16, hipStream_t stream);
void flowhip_corr_lookup_fwd_launch(const void* const* levels, const int* Hs,
                                    const int* Ws, const float* coords,
                                    void* out, int BP, int P,
                                    int L, int radius, int cl, int ldc,
                                    int is_bf16, hipStream_t stream);
bool flowhip_alt_corr_supported(int D, int radius, int L);
bool flowhip_alt_corr_lookup_fwd_launch(const void* f1,
                                        const void* const* levels,
                                        const int* Hs, const int* Ws,
                                        const float* coords, void* out,
                                        int BP, int P, int D, int L,
                                        int radius, int cl, int ldc,
                                        int out_bf16, hipStream_t stream);
bool flowhip_alt_corr_lookup_bwd_launch(
    const void* f1, const void* const* levels, float* const* accs,
    const int* Hs, const int* Ws, const float* coords, const void* grad,
    float* df1, float* df2, int B, int H, int W, int D, int L, int radius,
    int cl, int ldc, int g_bf16, int need_f1, int need_f2, int algo,
    hipStream_t stream);
void flowhip_corr_lookup_bwd_launch(const void* gout, const float* coords,
                                    void* const* glevels, const int* Hs,
                                    const int* Ws, int BP, int P,
                                    int L, int radius, int cl,
                                    int is_bf16, int acc,
                                    hipStream_t stream);
void flowhip_convex_up_fwd_launch(const float* flow, const float* mask,
                                  float* out, int N, int H, int W, int factor,
                                  hipStream_t stream);
void flowhip_convex_up_bwd_launch(const float* gout, const float* flow,
                                  const float* mask, float* gflow,
                                  float* gmask, float* contrib, int N, int H,
                                  int W, int factor, hipStream_t stream);
int flowhip_instnorm_partial_rows(int N, int C, long P);
void flowhip_transpose_cast_launch(const void* in, void* out, int B, int M,
                                   int N, int in_bf16, hipStream_t stream);
void flowhip_conf_pool_fwd_launch(const float* data, const float* conf,
                                  float* data_ds, float* conf_ds,
                                  unsigned char* code, long total, int H,
                                  int W, int OH, int OW, hipStream_t stream);
void flowhip_conf_pool_bwd_launch(const float* gdata_ds,
                                  const float* gconf_ds,
                                  const unsigned char* code, float* gdata,
                                  float* gconf, long total_in, int H, int W,
                                  int OH, int OW, hipStream_t stream);
void flowhip_instnorm_cl_fwd_launch(const void* x, void* y, float* mean,
                                    float* rstd, float* partials, int N,
                                    int C, long P, float eps, int is_bf16,
                                    bool deterministic, hipStream_t stream);
void flowhip_instnorm_cl_bwd_launch(const void* x, const void* dy,
                                    const float* mean, const float* rstd,
                                    float* gmean, float* gxmean,
                                    float* partials, void* dx, int N, int C,
                                    long P, int is_bf16, bool deterministic,
                                    hipStream_t stream);
void flowhip_zero_inject_fwd_launch(const float* inp, float* out, long total,
                                    int ih, int iw, int oh, int ow, int sH,
                                    int sW, hipStream_t stream);
void flowhip_zero_inject_bwd_launch(const float* gout, float* dinp,
                                    long total, int ih, int iw, int oh,
                                    int ow, int sH, int sW,
                                    hipStream_t stream);
void flowhip_forward_splat_plan(int H, int W, int splits, int* chunk_out,
                                int* G_out);
void flowhip_forward_splat_launch(const float* flow, float* out, double* ws_d,
                                  int* ws_i, int B, int H, int W, int chunk,
                                  int G, hipStream_t stream);
int flowhip_fb_consistency_blocks(int H, int W);
void flowhip_fb_consistency_launch(const float* flow_fw, const float* flow_bw,
                                   unsigned char* occ, float* res,
                                   double* partials, double* stats, int N,
                                   int H, int W, double alpha1, double alpha2,
                                   hipStream_t stream);
void flowhip_gru_gate1_fwd_launch(const void* zr, const void* h, void* z,
                                  void* rh, long total, int C, long P,
                                  int is_bf16, int cl, hipStream_t stream);
void flowhip_gru_gate1_bwd_launch(const void* dz, const void* drh,
                                  const void* zr, const void* h, void* dzr,
                                  void* dh, long total, int C, long P,
                                  int is_bf16, int cl, hipStream_t stream);
void flowhip_gru_gate2_fwd_launch(const void* qp, const void* z,
                                  const void* h, void* hnew, long total,
                                  int is_bf16, hipStream_t stream);
void flowhip_gru_gate2_bwd_launch(const void* dhnew, const void* qp,
                                  const void* z, const void* h, void* dqp,
                                  void* dz, void* dh, long total, int is_bf16,
                                  hipStream_t stream);
void flowhip_seq_loss_fwd_launch(const float* const* preds, int n,
                                 const float* gt, const float* valid,
                                 float* partials, float* out, long npix,
                                 long plane, float max_flow, float gamma,
                                 long numel_full, hipStream_t stream);
void flowhip_seq_loss_bwd_launch(const float* const* preds, float* const* dst,
                                 int n, const float* gt, const float* valid,
                                 const float* gloss, long npix, long plane,
                                 float max_flow, float gamma, long numel_full,
                                 hipStream_t stream);
bool flowhip_col_sum2_launch(const void* g, const void* x, float* out,
                             float* partials, long M, int C, int nchunk,
                             hipStream_t stream);
void flowhip_frozen_bn_apply_launch(const void* x, void* y, const float* s,
                                    const float* t, long M, int C,
                                    hipStream_t stream);
int flowhip_plane_dot_sum_pchunks(long P, int B, int C);
void flowhip_plane_dot_sum_launch(const float* x, const float* y,
                                  float* partials, float* out, long P, int B,
                                  int C, hipStream_t stream);
bool flowhip_col_sum_launch(const void* dy, float* out, float* partials,
                            long M, int C, int nchunk, hipStream_t stream);
void flowhip_up2x_cat_fwd_launch(const float* low, const float* skip,
                                 float* out, long total, int C1, int C2,
                                 int H, int W, hipStream_t stream);
void flowhip_area_up2x_fwd_launch(const float* in, float* out, long total,
                                  int H, int W, hipStream_t stream);
void flowhip_area_up2x_bwd_launch(const float* gout, float* gin,
                                  long total_in, int H, int W,
                                  hipStream_t stream);
bool flowhip_packernel_fwd_launch(const float* f, float* k, int B, int C,
                                  int H, int W, int K, int dil, int norm,
                                  hipStream_t stream);
bool flowhip_packernel_bwd_launch(const float* f, const float* k,
                                  const float* dk, float* df, int B, int C,
                                  int H, int W, int K, int dil, int norm,
                                  hipStream_t stream);
bool flowhip_pacconv_fwd_launch(const float* x, const float* kr,
                                const float* w, const float* bias, float* out,
                                int B, int Ci, int Co, int H, int W, int OH,
                                int OW, int pH, int pW, int K, int dil,
                                int shared, hipStream_t stream);
bool flowhip_pacconv_bwd_launch(const float* dy, const float* x,
                                const float* kr, const float* w, float* dx,
                                float* dk, float* partials, float* dw,
                                int nchunk, int B, int Ci, int Co, int H,
                                int W, int OH, int OW, int pH, int pW, int K,
                                int dil, int shared, hipStream_t stream);
void flowhip_pacpool_fwd_launch(const float* x, const float* kr, float* out,
                                int B, int C, int KCH, int H, int W, int OH,
                                int OW, int K, int sH, int sW, int pH,
                                int pW, int dil, hipStream_t stream);
void flowhip_pacpool_bwd_launch(const float* dy, const float* x,
                                const float* kr, float* dx, float* dk, int B,
                                int C, int KCH, int H, int W, int OH, int OW,
                                int K, int sH, int sW, int pH, int pW,
                                int dil, hipStream_t stream);
bool flowhip_corr_pyramid_fwd_launch(const void* corr, void* l1, void* l2,
                                     void* l3, int BP, int H0, int W0,
                                     int nlev, int is_bf16,
                                     hipStream_t stream);
bool flowhip_corr_pyramid_fits(int H0, int W0, int is_bf16);
void flowhip_corr_pyramid_bwd_launch(const void* g0, const void* g1,
                                     const void* g2, const void* g3,
                                     void* dcorr, long total, int H0, int W0,
                                     int is_bf16, hipStream_t stream);

namespace {

torch::Tensor bgemm_nt(torch::Tensor a, torch::Tensor b, double alpha,
                       bool out_bf16) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda(), "bgemm_nt: CUDA tensors required");
  TORCH_CHECK(a.dtype() == torch::kBFloat16 && b.dtype() == torch::kBFloat16,
              "bgemm_nt: bf16 operands required");
  TORCH_CHECK(a.dim() == 3 && b.dim() == 3, "bgemm_nt: (B,M,K) and (B,N,K)");
  TORCH_CHECK(a.is_contiguous() && b.is_contiguous());
  TORCH_CHECK(a.size(0) == b.size(0) && a.size(2) == b.size(2));
  TORCH_CHECK(a.size(2) % 64 == 0, "bgemm_nt: K must be a multiple of 64 "
              "(pad with zeros)");

  const int batch = a.size(0), M = a.size(1), N = b.size(1), K = a.size(2);
  auto c = torch::empty({batch, M, N},
                        a.options().dtype(out_bf16 ? torch::kBFloat16
                                                   : torch::kFloat32));
  const c10::cuda::CUDAGuard guard(a.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_bgemm_nt_launch(a.data_ptr(), b.data_ptr(), c.data_ptr(),
                          (float)alpha, batch, M, N, K, out_bf16 ? 1 : 0,
                          stream);
  return c;
}

torch::Tensor corr_lookup_fwd(std::vector<torch::Tensor> pyramid,
                              torch::Tensor coords, int64_t radius,
                              bool channels_last) {
  TORCH_CHECK(!pyramid.empty());
  TORCH_CHECK(coords.is_cuda() && coords.dtype() == torch::kFloat32 &&
              coords.is_contiguous());
  const int B = coords.size(0), H = coords.size(2), W = coords.size(3);
  const int P = H * W;
  const int L = (int)pyramid.size();
  const int K = 2 * (int)radius + 1;

  // channels-last: allocate with the channel count rounded up to 8 and
  // return a narrow view — the NHWC conv consumer reads whole 16-B pieces.
  // Output dtype follows the pyramid dtype (bf16-resident pyramid feeds
  // the bf16 motion-encoder conv with no cast pass).
  const bool bf = pyramid[0].dtype() == torch::kBFloat16;
  const auto odt = bf ? torch::kBFloat16 : torch::kFloat32;
  const long C = (long)L * K * K;
  const long C8 = channels_last ? (C + 7) / 8 * 8 : C;
  auto full = channels_last
                  ? torch::empty({B, C8, H, W},
                                 coords.options().dtype(odt)
                                     .memory_format(torch::MemoryFormat::ChannelsLast))
                  : torch::empty({B, C, H, W},
                                 coords.options().dtype(odt));
  auto out = (C8 != C) ? full.narrow(1, 0, C) : full;
  const c10::cuda::CUDAGuard guard(coords.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();

  const void* ptrs[4] = {nullptr, nullptr, nullptr, nullptr};
  int Hs[4] = {0, 0, 0, 0}, Ws[4] = {0, 0, 0, 0};
  TORCH_CHECK(L <= 4);
  for (int l = 0; l < L; ++l) {
    auto& lvl = pyramid[l];
    TORCH_CHECK(lvl.is_cuda() && lvl.is_contiguous() &&
                lvl.dtype() == (bf ? torch::kBFloat16 : torch::kFloat32),
                "corr_lookup: same-dtype contiguous pyramid levels required");
    TORCH_CHECK(lvl.size(0) == (long)B * P, "corr_lookup: level batch mismatch");
    ptrs[l] = lvl.data_ptr();
    Hs[l] = lvl.size(-2);
    Ws[l] = lvl.size(-1);
  }
  flowhip_corr_lookup_fwd_launch(
      ptrs, Hs, Ws, coords.data_ptr<float>(), full.data_ptr(), B * P, P, L,
      (int)radius, channels_last ? 1 : 0, (int)C8, bf ? 1 : 0, stream);
  return out;
}

// what algo == "auto" selects in alt_corr_lookup_bwd: 0 = direct, 1 = tiled
// (measured table in profiles/README.md, "On-demand correlation lookup")
#define ALT_CORR_BWD_AUTO_ALGO 1

bool alt_corr_supported(int64_t D, int64_t radius, int64_t L) {
  return flowhip_alt_corr_supported((int)D, (int)radius, (int)L);
}

// On-demand window lookup (alt_corr.hip): f1 (B,P,D) bf16 rows, levels =
// pooled f2 (B,Hl,Wl,D) bf16 channels-last. The emitted tensor (dtype,
// layout, 8-aligned channel stride) is the one corr_lookup_fwd emits.
torch::Tensor alt_corr_lookup_fwd(torch::Tensor f1,
                                  std::vector<torch::Tensor> levels,
                                  torch::Tensor coords, int64_t radius,
                                  bool channels_last, bool out_bf16) {
  TORCH_CHECK(!levels.empty() && levels.size() <= 4,
              "alt_corr_lookup: 1..4 levels");
  TORCH_CHECK(coords.is_cuda() && coords.dtype() == torch::kFloat32 &&
              coords.is_contiguous() && coords.dim() == 4 &&
              coords.size(1) == 2,
              "alt_corr_lookup: coords must be contiguous fp32 (B,2,H,W)");
  const int B = coords.size(0), H = coords.size(2), W = coords.size(3);
  const int P = H * W;
  const int L = (int)levels.size();
  const int K = 2 * (int)radius + 1;
  TORCH_CHECK(f1.is_cuda() && f1.dtype() == torch::kBFloat16 &&
              f1.is_contiguous() && f1.dim() == 3,
              "alt_corr_lookup: f1 must be contiguous bf16 (B,P,D)");
  TORCH_CHECK(f1.size(0) == B && f1.size(1) == P,
              "alt_corr_lookup: f1 / coords shape mismatch");
  const int D = f1.size(2);
  TORCH_CHECK(flowhip_alt_corr_supported(D, (int)radius, L),
              "alt_corr_lookup: unsupported D / radius / levels");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(f1.data_ptr()) & 15) == 0,
              "alt_corr_lookup: f1 must be 16-byte aligned");

  const void* ptrs[4] = {nullptr, nullptr, nullptr, nullptr};
  int Hs[4] = {0, 0, 0, 0}, Ws[4] = {0, 0, 0, 0};
  for (int l = 0; l < L; ++l) {
    auto& lvl = levels[l];
    TORCH_CHECK(lvl.is_cuda() && lvl.is_contiguous() &&
                lvl.dtype() == torch::kBFloat16 && lvl.dim() == 4,
                "alt_corr_lookup: contiguous bf16 (B,Hl,Wl,D) levels required");
    TORCH_CHECK(lvl.size(0) == B && lvl.size(3) == D,
                "alt_corr_lookup: level batch / channel mismatch");
    TORCH_CHECK(lvl.size(1) >= 1 && lvl.size(2) >= 1,
                "alt_corr_lookup: empty level");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(lvl.data_ptr()) & 15) == 0,
                "alt_corr_lookup: levels must be 16-byte aligned");
    ptrs[l] = lvl.data_ptr();
    Hs[l] = lvl.size(1);
    Ws[l] = lvl.size(2);
  }
  TORCH_CHECK(Hs[0] == H && Ws[0] == W,
              "alt_corr_lookup: level 0 must match the coords grid");

  const auto odt = out_bf16 ? torch::kBFloat16 : torch::kFloat32;
  const long C = (long)L * K * K;
  const long C8 = channels_last ? (C + 7) / 8 * 8 : C;
  auto full = channels_last
                  ? torch::empty({B, C8, H, W},
                                 coords.options().dtype(odt)
                                     .memory_format(torch::MemoryFormat::ChannelsLast))
                  : torch::empty({B, C, H, W},
                                 coords.options().dtype(odt));
  auto out = (C8 != C) ? full.narrow(1, 0, C) : full;
  const c10::cuda::CUDAGuard guard(coords.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  bool ok = flowhip_alt_corr_lookup_fwd_launch(
      f1.data_ptr(), ptrs, Hs, Ws, coords.data_ptr<float>(), full.data_ptr(),
      B * P, P, D, L, (int)radius, channels_last ? 1 : 0, (int)C8,
      out_bf16 ? 1 : 0, stream);
  TORCH_CHECK(ok, "alt_corr_lookup: unsupported configuration");
  return out;
}

// Backward of alt_corr_lookup_fwd (alt_corr_bwd.hip). `grad` has the layout
// of the forward's output: contiguous NCHW, or the NHWC view of rows with
// the 8-aligned stride (pad tail never read); fp32 or bf16. Returns
// (df1_rows (B,P,D) fp32 | None, df2 (B,D,H,W) fp32 channels-last | None).
// algo: "direct" (atomics per patch position), "tiled" (LDS box per 4x4
// pixel tile) or "auto" (the measured pick, profiles/README.md).
std::tuple<c10::optional<torch::Tensor>, c10::optional<torch::Tensor>>
alt_corr_lookup_bwd(torch::Tensor grad, torch::Tensor f1,
                    std::vector<torch::Tensor> levels, torch::Tensor coords,
                    int64_t radius, bool channels_last, bool need_f1,
                    bool need_f2, const std::string& algo) {
  TORCH_CHECK(!levels.empty() && levels.size() <= 4,
              "alt_corr_lookup_bwd: 1..4 levels");
  TORCH_CHECK(coords.is_cuda() && coords.dtype() == torch::kFloat32 &&
              coords.is_contiguous() && coords.dim() == 4 &&
              coords.size(1) == 2,
              "alt_corr_lookup_bwd: coords must be contiguous fp32 (B,2,H,W)");
  const int B = coords.size(0), H = coords.size(2), W = coords.size(3);
  const int P = H * W;
  const int L = (int)levels.size();
  const int K = 2 * (int)radius + 1;
  TORCH_CHECK(f1.is_cuda() && f1.dtype() == torch::kBFloat16 &&
              f1.is_contiguous() && f1.dim() == 3,
              "alt_corr_lookup_bwd: f1 must be contiguous bf16 (B,P,D)");
  TORCH_CHECK(f1.size(0) == B && f1.size(1) == P,
              "alt_corr_lookup_bwd: f1 / coords shape mismatch");
  const int D = f1.size(2);
  TORCH_CHECK(flowhip_alt_corr_supported(D, (int)radius, L),
              "alt_corr_lookup_bwd: unsupported D / radius / levels");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(f1.data_ptr()) & 15) == 0,
              "alt_corr_lookup_bwd: f1 must be 16-byte aligned");

  const void* ptrs[4] = {nullptr, nullptr, nullptr, nullptr};
  int Hs[4] = {0, 0, 0, 0}, Ws[4] = {0, 0, 0, 0};
  int64_t cells = 0;
  for (int l = 0; l < L; ++l) {
    auto& lvl = levels[l];
    TORCH_CHECK(lvl.is_cuda() && lvl.is_contiguous() &&
                lvl.dtype() == torch::kBFloat16 && lvl.dim() == 4,
                "alt_corr_lookup_bwd: contiguous bf16 (B,Hl,Wl,D) levels "
                "required");
    TORCH_CHECK(lvl.size(0) == B && lvl.size(3) == D,
                "alt_corr_lookup_bwd: level batch / channel mismatch");
    TORCH_CHECK(lvl.size(1) >= 1 && lvl.size(2) >= 1,
                "alt_corr_lookup_bwd: empty level");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(lvl.data_ptr()) & 15) == 0,
                "alt_corr_lookup_bwd: levels must be 16-byte aligned");
    ptrs[l] = lvl.data_ptr();
    Hs[l] = lvl.size(1);
    Ws[l] = lvl.size(2);
    cells += (int64_t)B * Hs[l] * Ws[l];
  }
  TORCH_CHECK(Hs[0] == H && Ws[0] == W,
              "alt_corr_lookup_bwd: level 0 must match the coords grid");

  const int64_t C = (int64_t)L * K * K;
  const int64_t C8 = channels_last ? (C + 7) / 8 * 8 : C;
  const bool g_bf16 = grad.dtype() == torch::kBFloat16;
  TORCH_CHECK(grad.is_cuda() && (g_bf16 || grad.dtype() == torch::kFloat32),
              "alt_corr_lookup_bwd: grad must be fp32 or bf16 on the GPU");
  TORCH_CHECK(grad.dim() == 4 && grad.size(0) == B && grad.size(1) == C &&
              grad.size(2) == H && grad.size(3) == W,
              "alt_corr_lookup_bwd: grad must be (B, L*K*K, H, W)");
  if (channels_last) {
    TORCH_CHECK(grad.stride(1) == 1 && grad.stride(3) == C8 &&
                grad.stride(2) == (int64_t)W * C8 &&
                (B == 1 || grad.stride(0) == (int64_t)P * C8),
                "alt_corr_lookup_bwd: grad must have the forward output's "
                "NHWC strides (8-aligned channel stride)");
  } else {
    TORCH_CHECK(grad.is_contiguous(),
                "alt_corr_lookup_bwd: grad must be contiguous NCHW");
  }
  int algo_id;
  if (algo == "direct") {
    algo_id = 0;
  } else if (algo == "tiled") {
    algo_id = 1;
  } else {
    TORCH_CHECK(algo == "auto", "alt_corr_lookup_bwd: algo must be auto, "
                "direct or tiled");
    algo_id = ALT_CORR_BWD_AUTO_ALGO;
  }

  const c10::cuda::CUDAGuard guard(coords.device());
  const auto fopt = coords.options().dtype(torch::kFloat32);
  c10::optional<torch::Tensor> df1, df2;
  torch::Tensor d1, d2, acc;
  float* accs[4] = {nullptr, nullptr, nullptr, nullptr};
  if (need_f1) d1 = torch::empty({B, P, D}, fopt);
  if (need_f2) {
    d2 = torch::empty({B, H, W, D}, fopt);
    // one zero-initialised allocation holds every level's accumulator
    acc = torch::zeros({cells * D}, fopt);
    int64_t off = 0;
    for (int l = 0; l < L; ++l) {
      accs[l] = acc.data_ptr<float>() + off;
      off += (int64_t)B * Hs[l] * Ws[l] * D;
    }
  }
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  bool ok = flowhip_alt_corr_lookup_bwd_launch(
      f1.data_ptr(), ptrs, accs, Hs, Ws, coords.data_ptr<float>(),
      grad.data_ptr(), need_f1 ? d1.data_ptr<float>() : nullptr,
      need_f2 ? d2.data_ptr<float>() : nullptr, B, H, W, D, L, (int)radius,
      channels_last ? 1 : 0, (int)C8, g_bf16 ? 1 : 0, need_f1 ? 1 : 0,
      need_f2 ? 1 : 0, algo_id, stream);
  TORCH_CHECK(ok, "alt_corr_lookup_bwd: unsupported configuration");
  if (need_f1) df1 = d1;
  if (need_f2) df2 = d2.permute({0, 3, 1, 2});
  return {df1, df2};
}

std::vector<torch::Tensor> corr_lookup_bwd(torch::Tensor gout,
                                           torch::Tensor coords,
                                           int64_t radius,
                                           std::vector<std::vector<int64_t>>
                                               level_shapes,
                                           bool channels_last,
                                           bool levels_bf16,
                                           c10::optional<std::vector<torch::Tensor>>
                                               prev) {
  TORCH_CHECK(gout.is_cuda() &&
              gout.dtype() == (levels_bf16 ? torch::kBFloat16
                                           : torch::kFloat32),
              "corr_lookup_bwd: gout dtype must match the pyramid dtype");
  TORCH_CHECK(channels_last
                  ? gout.is_contiguous(torch::MemoryFormat::ChannelsLast)
                  : gout.is_contiguous());
  const int B = coords.size(0), H = coords.size(2), W = coords.size(3);
  const int P = H * W;
  const int L = (int)level_shapes.size();

  const c10::cuda::CUDAGuard guard(coords.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();

  // `prev` = the NEXT iteration's level grads (the pyramid is threaded
  // through the iteration loop as a chain): accumulate this lookup's
  // contribution into them IN KERNEL — no fresh zero-fill, no autograd
  // fan-in add_. Without prev: one flat zero-fill for all levels, plain
  // stores. Level-grad dtype matches the resident pyramid dtype.
  std::vector<torch::Tensor> grads;
  grads.reserve(L);
  const bool acc = prev.has_value();
  if (acc) {
    TORCH_CHECK((int)prev->size() == L);
    for (int l = 0; l < L; ++l) {
      auto& g = (*prev)[l];
      TORCH_CHECK(g.is_cuda() && g.is_contiguous() &&
                  g.dtype() == gout.dtype());
      grads.push_back(g);
    }
  } else {
    int64_t total = 0;
    std::vector<int64_t> sizes(L);
    for (int l = 0; l < L; ++l) {
      int64_t n = 1;
      for (auto d : level_shapes[l]) n *= d;
      sizes[l] = n;
      total += n;
    }
    auto flat = torch::zeros(
        {total}, gout.options().dtype(levels_bf16 ? torch::kBFloat16
                                                  : torch::kFloat32));
    int64_t off = 0;
    for (int l = 0; l < L; ++l) {
      grads.push_back(flat.narrow(0, off, sizes[l]).view(level_shapes[l]));
      off += sizes[l];
    }
  }
  void* gptrs[4] = {nullptr, nullptr, nullptr, nullptr};
  int Hs[4] = {0, 0, 0, 0}, Ws[4] = {0, 0, 0, 0};
  TORCH_CHECK(L <= 4);
  for (int l = 0; l < L; ++l) {
    gptrs[l] = grads[l].data_ptr();
    Hs[l] = grads[l].size(-2);
    Ws[l] = grads[l].size(-1);
  }
  flowhip_corr_lookup_bwd_launch(
      gout.data_ptr(), coords.data_ptr<float>(), gptrs, Hs, Ws,
      B * P, P, L, (int)radius, channels_last ? 1 : 0,
      levels_bf16 ? 1 : 0, acc ? 1 : 0, stream);
  return grads;
}

std::vector<torch::Tensor> corr_pyramid_fwd(torch::Tensor corr,
                                            int64_t num_levels) {
  const bool bf = corr.dtype() == torch::kBFloat16;
  TORCH_CHECK(corr.is_cuda() && (bf || corr.dtype() == torch::kFloat32) &&
              corr.is_contiguous());
  TORCH_CHECK(corr.dim() == 4 && corr.size(1) == 1);
  const long BP = corr.size(0);
  const int H0 = corr.size(2), W0 = corr.size(3);
  int H = H0, W = W0;
  std::vector<torch::Tensor> levels;
  for (int l = 1; l < num_levels; ++l) {
    H /= 2; W /= 2;
    levels.push_back(torch::empty({BP, 1, H, W}, corr.options()));
  }
  const c10::cuda::CUDAGuard guard(corr.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  void* p1 = levels.size() > 0 ? levels[0].data_ptr() : nullptr;
  void* p2 = levels.size() > 1 ? levels[1].data_ptr() : nullptr;
  void* p3 = levels.size() > 2 ? levels[2].data_ptr() : nullptr;
  bool ok = flowhip_corr_pyramid_fwd_launch(
      corr.data_ptr(), p1, p2, p3, (int)BP, H0, W0, (int)num_levels,
      bf ? 1 : 0, stream);
  TORCH_CHECK(ok, "corr_pyramid_fwd: unsupported shape (fall back to torch)");
  return levels;
}

bool corr_pyramid_fits(int64_t H0, int64_t W0, bool bf16) {
  return flowhip_corr_pyramid_fits((int)H0, (int)W0, bf16 ? 1 : 0);
}

torch::Tensor corr_pyramid_bwd(std::vector<c10::optional<torch::Tensor>> grads,
                               std::vector<int64_t> corr_shape) {
  TORCH_CHECK(grads.size() >= 1 && grads.size() <= 4);
  const long BP = corr_shape[0];
  const int H0 = corr_shape[2], W0 = corr_shape[3];
  const void* g[4] = {nullptr, nullptr, nullptr, nullptr};
  torch::TensorOptions opts;
  torch::Device dev(torch::kCUDA);
  bool have = false, bf = false;
  for (size_t l = 0; l < grads.size(); ++l) {
    if (grads[l].has_value()) {
      auto& t = grads[l].value();
      const bool tb = t.dtype() == torch::kBFloat16;
      TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  (tb || t.dtype() == torch::kFloat32));
      if (have) TORCH_CHECK(tb == bf, "corr_pyramid_bwd: mixed grad dtypes");
      g[l] = t.data_ptr();
      opts = t.options();
      dev = t.device();
      have = true;
      bf = tb;
    }
  }
  TORCH_CHECK(have, "corr_pyramid_bwd: all grads missing");
  auto dcorr = torch::empty(corr_shape, opts);
  const c10::cuda::CUDAGuard guard(dev);
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_corr_pyramid_bwd_launch(g[0], g[1], g[2], g[3],
                                  dcorr.data_ptr(),
                                  (long)BP * H0 * W0, H0, W0, bf ? 1 : 0,
                                  stream);
  return dcorr;
}

torch::Tensor convex_up_fwd(torch::Tensor flow, torch::Tensor mask,
                            int64_t factor) {
  TORCH_CHECK(flow.is_cuda() && flow.dtype() == torch::kFloat32 &&
              flow.is_contiguous());
  TORCH_CHECK(mask.is_cuda() && mask.dtype() == torch::kFloat32 &&
              mask.is_contiguous());
  TORCH_CHECK(factor == 8, "convex_up: factor 8 only");
  const int N = flow.size(0), H = flow.size(2), W = flow.size(3);
  TORCH_CHECK(flow.size(1) == 2 && mask.size(1) == 9 * factor * factor);

  auto out = torch::empty({N, 2, factor * H, factor * W}, flow.options());
  const c10::cuda::CUDAGuard guard(flow.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_convex_up_fwd_launch(flow.data_ptr<float>(), mask.data_ptr<float>(),
                               out.data_ptr<float>(), N, H, W, (int)factor,
                               stream);
  return out;
}

std::vector<torch::Tensor> convex_up_bwd(torch::Tensor gout,
                                         torch::Tensor flow,
                                         torch::Tensor mask, int64_t factor,
                                         bool deterministic) {
  TORCH_CHECK(gout.is_cuda() && gout.is_contiguous() &&
              gout.dtype() == torch::kFloat32);
  const int N = flow.size(0), H = flow.size(2), W = flow.size(3);
  // deterministic: per-pixel tap sums go to a scratch that a second kernel
  // gathers in a fixed order; nothing is accumulated in place
  auto gflow = deterministic ? torch::empty_like(flow)
                             : torch::zeros_like(flow);
  torch::Tensor contrib;
  if (deterministic)
    contrib = torch::empty({(long)N, (long)H, (long)W, 8, 9, 2},
                           flow.options());
  auto gmask = torch::empty_like(mask);
  const c10::cuda::CUDAGuard guard(flow.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_convex_up_bwd_launch(gout.data_ptr<float>(), flow.data_ptr<float>(),
                               mask.data_ptr<float>(),
                               gflow.data_ptr<float>(),
                               gmask.data_ptr<float>(),
                               deterministic ? contrib.data_ptr<float>()
                                             : nullptr,
                               N, H, W, (int)factor, stream);
  return {gflow, gmask};
}

// The one place a normalized-convolution binding turns its tensors into an
// NConvGeom: data (N, Ci, H, W) and weight (Co, Ci, K, K) on the device,
// fp32, contiguous, agreeing on Ci, inside the kernels' envelope.
#define FLOWHIP_NCONV_ENVELOPE_MSG                                          \
  ": outside the normalized-convolution kernels' envelope: (K, Ci, Co) "    \
  "must be an entry of FLOWHIP_NCONV_TABLE (csrc/nconv.h) and W % 4 == 0"

bool nconv_is_plane(const torch::Tensor& t) {
  return t.is_cuda() && t.is_contiguous() && t.dtype() == torch::kFloat32 &&
         t.dim() == 4;
}

NConvGeom nconv_geom(const char* who, const torch::Tensor& data,
                     const torch::Tensor& weight) {
  TORCH_CHECK(nconv_is_plane(data) && nconv_is_plane(weight) &&
                  weight.size(1) == data.size(1) &&
                  weight.size(3) == weight.size(2),
              who, ": data (N,Ci,H,W) and weight (Co,Ci,K,K) must be "
              "contiguous fp32 device tensors");
  const NConvGeom g{(int)data.size(0),   (int)data.size(1),
                    (int)weight.size(0), (int)data.size(2),
                    (int)data.size(3),   (int)weight.size(2)};
  TORCH_CHECK(flowhip_nconv_launchable(g), who, FLOWHIP_NCONV_ENVELOPE_MSG,
              "; got K=", g.K, " Ci=", g.Ci, " Co=", g.Co, " W=", g.W);
  return g;
}

// t is a (N, C, H, W) plane stack of the layer g
void nconv_check_planes(const char* who, const NConvGeom& g,
                        const torch::Tensor& t, int C) {
  TORCH_CHECK(nconv_is_plane(t) && t.size(0) == g.N && t.size(1) == C &&
                  t.size(2) == g.H && t.size(3) == g.W,
              who, ": expected a contiguous fp32 (", g.N, ",", C, ",", g.H,
              ",", g.W, ") device tensor");
}

const float* nconv_bias_ptr(const char* who, const NConvGeom& g,
                            const c10::optional<torch::Tensor>& bias) {
  if (!bias.has_value()) return nullptr;
  TORCH_CHECK(bias->is_cuda() && bias->is_contiguous() &&
                  bias->dtype() == torch::kFloat32 && bias->numel() == g.Co,
              who, ": bias must be a contiguous fp32 (Co) device tensor");
  return bias->data_ptr<float>();
}

std::vector<torch::Tensor> nconv_fwd(torch::Tensor data, torch::Tensor conf,
                                     torch::Tensor weight,
                                     c10::optional<torch::Tensor> bias) {
  const NConvGeom g = nconv_geom("nconv_fwd", data, weight);
  nconv_check_planes("nconv_fwd", g, conf, g.Ci);
  const float* bptr = nconv_bias_ptr("nconv_fwd", g, bias);
  auto out = torch::empty({g.N, g.Co, g.H, g.W}, data.options());
  auto cout = torch::empty({g.N, g.Co, g.H, g.W}, data.options());
  const c10::cuda::CUDAGuard guard(data.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  const bool ok = flowhip_nconv_fwd_launch(
      data.data_ptr<float>(), conf.data_ptr<float>(),
      weight.data_ptr<float>(), bptr, out.data_ptr<float>(),
      cout.data_ptr<float>(), g, stream);
  TORCH_CHECK(ok, "nconv_fwd: launch refused a checked geometry");
  return {out, cout};
}

std::vector<torch::Tensor> nconv_bwd(torch::Tensor dnomin,
                                     torch::Tensor ddenom, torch::Tensor data,
                                     torch::Tensor conf,
                                     torch::Tensor weight) {
  const NConvGeom g = nconv_geom("nconv_bwd", data, weight);
  nconv_check_planes("nconv_bwd", g, conf, g.Ci);
  nconv_check_planes("nconv_bwd", g, dnomin, g.Co);
  nconv_check_planes("nconv_bwd", g, ddenom, g.Co);

  auto ddata = torch::empty_like(data);
  auto dconf = torch::empty_like(conf);
  auto dweight = torch::empty_like(weight);
  auto partials = torch::empty(
      {flowhip_nconv_wrw_nblocks(g), (long)g.Co * g.Ci * g.K * g.K},
      data.options());
  const c10::cuda::CUDAGuard guard(data.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  const bool ok =
      flowhip_nconv_bwd_data_launch(
          dnomin.data_ptr<float>(), ddenom.data_ptr<float>(),
          data.data_ptr<float>(), conf.data_ptr<float>(),
          weight.data_ptr<float>(), ddata.data_ptr<float>(),
          dconf.data_ptr<float>(), g, stream) &&
      flowhip_nconv_wrw_launch(
          dnomin.data_ptr<float>(), ddenom.data_ptr<float>(),
          data.data_ptr<float>(), conf.data_ptr<float>(),
          partials.data_ptr<float>(), dweight.data_ptr<float>(), g, stream);
  TORCH_CHECK(ok, "nconv_bwd: launch refused a checked geometry");
  return {ddata, dconf, dweight};
}

// Elementwise, with no data / weight to take (K, Ci) from, so the table is
// not consulted here. It refuses W % 4 != 0 only so that no binding of the
// family accepts planes the others refuse.
std::vector<torch::Tensor> nconv_bwd_prep(
    torch::Tensor gout, c10::optional<torch::Tensor> gcout, torch::Tensor out,
    torch::Tensor cout, torch::Tensor wsum, c10::optional<torch::Tensor> bias,
    double eps) {
  TORCH_CHECK(nconv_is_plane(gout), "nconv_bwd_prep: gout must be a "
              "contiguous fp32 (N,Co,H,W) device tensor");
  const NConvGeom g{(int)gout.size(0), 0, (int)gout.size(1),
                    (int)gout.size(2), (int)gout.size(3), 0};
  TORCH_CHECK(g.W % 4 == 0, "nconv_bwd_prep: W % 4 == 0 required, as by every "
              "normalized-convolution binding (the kernel table is not "
              "checked here: this step sees no K or Ci); got W=", g.W);
  nconv_check_planes("nconv_bwd_prep", g, out, g.Co);
  nconv_check_planes("nconv_bwd_prep", g, cout, g.Co);
  if (gcout.has_value()) nconv_check_planes("nconv_bwd_prep", g, *gcout, g.Co);
  TORCH_CHECK(wsum.is_cuda() && wsum.is_contiguous() &&
                  wsum.dtype() == torch::kFloat32 && wsum.numel() == g.Co,
              "nconv_bwd_prep: wsum must be a contiguous fp32 (Co) device "
              "tensor");
  const float* bptr = nconv_bias_ptr("nconv_bwd_prep", g, bias);
  auto dnomin = torch::empty_like(gout);
  auto ddenom = torch::empty_like(gout);
  const c10::cuda::CUDAGuard guard(gout.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_nconv_bwd_prep_launch(
      gout.data_ptr<float>(),
      gcout.has_value() ? gcout->data_ptr<float>() : nullptr,
      out.data_ptr<float>(), cout.data_ptr<float>(), wsum.data_ptr<float>(),
      bptr, dnomin.data_ptr<float>(), ddenom.data_ptr<float>(), gout.numel(),
      (long)g.H * g.W, g.Co, (float)eps, stream);
  return {dnomin, ddenom};
}

torch::Tensor seq_loss_fwd(std::vector<torch::Tensor> preds,
                           torch::Tensor gt, torch::Tensor valid,
                           double gamma, double max_flow) {
  const int n = (int)preds.size();
  TORCH_CHECK(n >= 1 && n <= 32, "seq_loss: 1..32 predictions");
  TORCH_CHECK(gt.is_cuda() && gt.is_contiguous() &&
              gt.dtype() == torch::kFloat32);
  TORCH_CHECK(valid.is_cuda() && valid.is_contiguous());
  const long B = gt.size(0), H = gt.size(2), W = gt.size(3);
  const long plane = H * W, npix = B * plane;
  std::vector<const float*> ptrs(n);
  for (int i = 0; i < n; ++i) {
    TORCH_CHECK(preds[i].is_cuda() && preds[i].is_contiguous() &&
                preds[i].dtype() == torch::kFloat32 &&
                preds[i].sizes() == gt.sizes());
    ptrs[i] = preds[i].data_ptr<float>();
  }
  auto partials = torch::empty({1024, (long)n + 5},
                               gt.options().dtype(torch::kFloat32));
  auto out = torch::empty({5}, gt.options().dtype(torch::kFloat32));
  const c10::cuda::CUDAGuard guard(gt.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_seq_loss_fwd_launch(ptrs.data(), n, gt.data_ptr<float>(),
                              valid.data_ptr<float>(),
                              partials.data_ptr<float>(),
                              out.data_ptr<float>(), npix, plane,
                              (float)max_flow, (float)gamma, gt.numel(),
                              stream);
  return out;
}

std::vector<torch::Tensor> seq_loss_bwd(std::vector<torch::Tensor> preds,
                                        torch::Tensor gt, torch::Tensor valid,
                                        torch::Tensor gloss, double gamma,
                                        double max_flow) {
  const int n = (int)preds.size();
  const long B = gt.size(0), H = gt.size(2), W = gt.size(3);
  const long plane = H * W, npix = B * plane;
  std::vector<const float*> ptrs(n);
  std::vector<float*> gptrs(n);
  std::vector<torch::Tensor> grads;
  grads.reserve(n);
  for (int i = 0; i < n; ++i) {
    ptrs[i] = preds[i].data_ptr<float>();
    grads.push_back(torch::empty_like(preds[i]));
    gptrs[i] = grads[i].data_ptr<float>();
  }
  const c10::cuda::CUDAGuard guard(gt.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_seq_loss_bwd_launch(ptrs.data(), gptrs.data(), n,
                              gt.data_ptr<float>(), valid.data_ptr<float>(),
                              gloss.data_ptr<float>(), npix, plane,
                              (float)max_flow, (float)gamma, gt.numel(),
                              stream);
  return grads;
}

namespace gg {

bool is_cl(const torch::Tensor& t) {
  return t.is_contiguous(torch::MemoryFormat::ChannelsLast);
}

torch::Tensor make_like(const torch::Tensor& t, bool cl) {
  return cl ? torch::empty(t.sizes(), t.options(),
                           torch::MemoryFormat::ChannelsLast)
            : torch::empty(t.sizes(), t.options());
}

}  // namespace gg

std::vector<torch::Tensor> gru_gate1_fwd(torch::Tensor zr, torch::Tensor h) {
  TORCH_CHECK(zr.is_cuda() && h.is_cuda());
  TORCH_CHECK(zr.scalar_type() == h.scalar_type());
  const bool bf16 = zr.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || zr.scalar_type() == torch::kFloat32);
  const bool cl = gg::is_cl(zr);
  TORCH_CHECK(cl ? gg::is_cl(h) : h.is_contiguous(),
              "gru_gate1: layouts must match");
  const int C = h.size(1);
  const long P = (long)h.size(2) * h.size(3);
  TORCH_CHECK(zr.size(1) == 2 * C && zr.size(0) == h.size(0));
  auto z = gg::make_like(h, cl);
  auto rh = gg::make_like(h, cl);
  const c10::cuda::CUDAGuard guard(h.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_gru_gate1_fwd_launch(zr.data_ptr(), h.data_ptr(), z.data_ptr(),
                               rh.data_ptr(), h.numel(), C, P, bf16 ? 1 : 0,
                               cl ? 1 : 0, stream);
  return {z, rh};
}

std::vector<torch::Tensor> gru_gate1_bwd(c10::optional<torch::Tensor> dz,
                                         torch::Tensor drh, torch::Tensor zr,
                                         torch::Tensor h) {
  const bool bf16 = zr.scalar_type() == torch::kBFloat16;
  const bool cl = gg::is_cl(zr);
  const int C = h.size(1);
  const long P = (long)h.size(2) * h.size(3);
  auto dzr = gg::make_like(zr, cl);
  auto dh = gg::make_like(h, cl);
  const c10::cuda::CUDAGuard guard(h.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_gru_gate1_bwd_launch(
      dz.has_value() ? dz->data_ptr() : nullptr, drh.data_ptr(),
      zr.data_ptr(), h.data_ptr(), dzr.data_ptr(), dh.data_ptr(), h.numel(),
      C, P, bf16 ? 1 : 0, cl ? 1 : 0, stream);
  return {dzr, dh};
}

torch::Tensor gru_gate2_fwd(torch::Tensor qp, torch::Tensor z,
                            torch::Tensor h) {
  const bool bf16 = qp.scalar_type() == torch::kBFloat16;
  const bool cl = gg::is_cl(qp);
  auto hnew = gg::make_like(h, cl);
  const c10::cuda::CUDAGuard guard(h.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_gru_gate2_fwd_launch(qp.data_ptr(), z.data_ptr(), h.data_ptr(),
                               hnew.data_ptr(), h.numel(), bf16 ? 1 : 0,
                               stream);
  return hnew;
}

std::vector<torch::Tensor> gru_gate2_bwd(torch::Tensor dhnew,
                                         torch::Tensor qp, torch::Tensor z,
                                         torch::Tensor h) {
  const bool bf16 = qp.scalar_type() == torch::kBFloat16;
  const bool cl = gg::is_cl(qp);
  auto dqp = gg::make_like(qp, cl);
  auto dz = gg::make_like(z, cl);
  auto dh = gg::make_like(h, cl);
  const c10::cuda::CUDAGuard guard(h.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_gru_gate2_bwd_launch(dhnew.data_ptr(), qp.data_ptr(), z.data_ptr(),
                               h.data_ptr(), dqp.data_ptr(), dz.data_ptr(),
                               dh.data_ptr(), h.numel(), bf16 ? 1 : 0,
                               stream);
  return {dqp, dz, dh};
}

torch::Tensor zero_inject_fwd(torch::Tensor inp, int64_t sH, int64_t sW,
                              int64_t oh, int64_t ow) {
  TORCH_CHECK(inp.is_cuda() && inp.dtype() == torch::kFloat32);
  auto x = inp.contiguous();
  const long N = x.size(0), C = x.size(1);
  const int ih = x.size(2), iw = x.size(3);
  auto out = torch::empty({N, C, oh, ow}, x.options());
  const c10::cuda::CUDAGuard guard(x.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_zero_inject_fwd_launch(x.data_ptr<float>(), out.data_ptr<float>(),
                                 out.numel(), ih, iw, (int)oh, (int)ow,
                                 (int)sH, (int)sW, stream);
  return out;
}

torch::Tensor zero_inject_bwd(torch::Tensor gout, int64_t sH, int64_t sW,
                              int64_t ih, int64_t iw) {
  auto g = gout.contiguous();
  const long N = g.size(0), C = g.size(1);
  const int oh = g.size(2), ow = g.size(3);
  auto dinp = torch::empty({N, C, ih, iw}, g.options());
  const c10::cuda::CUDAGuard guard(g.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_zero_inject_bwd_launch(g.data_ptr<float>(), dinp.data_ptr<float>(),
                                 dinp.numel(), (int)ih, (int)iw, oh, ow,
                                 (int)sH, (int)sW, stream);
  return dinp;
}

// The search kernel indexes targets and sources with int and overshoots the
// last tile by up to one tile of targets.
static void forward_splat_check_hw(int64_t H, int64_t W) {
  TORCH_CHECK(H >= 1 && W >= 1 && H * W < (int64_t(1) << 31) - 4096,
              "forward_splat: H*W must stay below 2^31");
}

// Chunk count G the splat picks for an (H, W) field (splits = 0), or the one
// a forced `splits` comes to once no chunk is left empty.
int64_t forward_splat_plan(int64_t H, int64_t W, int64_t splits) {
  forward_splat_check_hw(H, W);
  TORCH_CHECK(splits >= 0, "forward_splat: splits must be >= 0 (0 = planned)");
  int chunk, G;
  flowhip_forward_splat_plan((int)H, (int)W,
                             (int)std::min<int64_t>(splits, H * W), &chunk,
                             &G);
  return G;
}

// Nearest-neighbour forward splat, (B,2,H,W) fp32 -> (B,2,H,W) fp32.
// splits: 0 = planned chunk count, otherwise forced (1 = single pass that
// writes the output directly, > 1 = partials + finish kernel).
torch::Tensor forward_splat(torch::Tensor flow, int64_t splits) {
  TORCH_CHECK(flow.is_cuda() && flow.dtype() == torch::kFloat32 &&
                  flow.dim() == 4 && flow.size(1) == 2,
              "forward_splat: (B,2,H,W) fp32 CUDA tensor required");
  TORCH_CHECK(splits >= 0, "forward_splat: splits must be >= 0 (0 = planned)");
  auto x = flow.contiguous();
  const int64_t B = x.size(0), H = x.size(2), W = x.size(3);
  auto out = torch::empty_like(x);
  if (B == 0 || H == 0 || W == 0) return out;
  forward_splat_check_hw(H, W);
  TORCH_CHECK(B <= 65535, "forward_splat: batch exceeds the grid limit");
  int chunk, G;
  flowhip_forward_splat_plan((int)H, (int)W,
                             (int)std::min<int64_t>(splits, H * W), &chunk,
                             &G);
  torch::Tensor ws_d, ws_i;
  if (G > 1) {
    ws_d = torch::empty({B, (int64_t)G, H * W},
                        x.options().dtype(torch::kFloat64));
    ws_i = torch::empty({B, (int64_t)G, H * W},
                        x.options().dtype(torch::kInt32));
  }
  const c10::cuda::CUDAGuard guard(x.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_forward_splat_launch(
      x.data_ptr<float>(), out.data_ptr<float>(),
      G > 1 ? ws_d.data_ptr<double>() : nullptr,
      G > 1 ? ws_i.data_ptr<int>() : nullptr, (int)B, (int)H, (int)W, chunk,
      G, stream);
  return out;
}

// Forward-backward consistency of a bidirectional flow pair, both directions
// in one launch: two (N,2,H,W) fp32 flows -> {occ_fw, occ_bw} uint8 (N,1,H,W),
// {res_fw, res_bw} fp32 (N,1,H,W), stats fp64 (N,2,4).
std::vector<torch::Tensor> fb_consistency(torch::Tensor flow_fw,
                                          torch::Tensor flow_bw, double alpha1,
                                          double alpha2) {
  TORCH_CHECK(flow_fw.is_cuda() && flow_bw.is_cuda() &&
                  flow_fw.device() == flow_bw.device() &&
                  flow_fw.dtype() == torch::kFloat32 &&
                  flow_bw.dtype() == torch::kFloat32 && flow_fw.dim() == 4 &&
                  flow_fw.size(1) == 2 && flow_fw.sizes() == flow_bw.sizes(),
              "fb_consistency: two (N,2,H,W) fp32 CUDA tensors of one shape "
              "required");
  auto f = flow_fw.contiguous();
  auto b = flow_bw.contiguous();
  const int64_t N = f.size(0), H = f.size(2), W = f.size(3);
  TORCH_CHECK(H >= 2 && W >= 2, "fb_consistency: H and W must be >= 2");
  // the kernel indexes a plane with int and overshoots it by up to one
  // workgroup of pixels
  TORCH_CHECK(H * W < (int64_t(1) << 31) - 4096,
              "fb_consistency: H*W must stay below 2^31");
  TORCH_CHECK(N <= 65535, "fb_consistency: batch exceeds the grid limit");
  auto occ = torch::empty({2, N, 1, H, W}, f.options().dtype(torch::kUInt8));
  auto res = torch::empty({2, N, 1, H, W}, f.options());
  auto stats = torch::empty({N, 2, 4}, f.options().dtype(torch::kFloat64));
  if (N > 0) {
    const int nblk = flowhip_fb_consistency_blocks((int)H, (int)W);
    auto partials = torch::empty({2, N, (int64_t)nblk, 4}, stats.options());
    const c10::cuda::CUDAGuard guard(f.device());
    hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
    flowhip_fb_consistency_launch(
        f.data_ptr<float>(), b.data_ptr<float>(), occ.data_ptr<uint8_t>(),
        res.data_ptr<float>(), partials.data_ptr<double>(),
        stats.data_ptr<double>(), (int)N, (int)H, (int)W, alpha1, alpha2,
        stream);
  }
  return {occ[0], occ[1], res[0], res[1], stats};
}

std::vector<torch::Tensor> instnorm_cl_fwd(torch::Tensor x, double eps,
                                           bool deterministic) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4);
  TORCH_CHECK(x.is_contiguous(torch::MemoryFormat::ChannelsLast),
              "instnorm_cl: channels_last input required");
  const bool bf16 = x.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || x.scalar_type() == torch::kFloat32);
  const int N = x.size(0), C = x.size(1);
  const long P = (long)x.size(2) * x.size(3);
  auto y = torch::empty(x.sizes(), x.options(),
                        torch::MemoryFormat::ChannelsLast);
  auto mean = torch::empty({(long)N, (long)C},
                           x.options().dtype(torch::kFloat32));
  auto rstd = torch::empty_like(mean);
  auto partials = torch::empty({(long)flowhip_instnorm_partial_rows(N, C, P),
                                64},
                               x.options().dtype(torch::kFloat32));
  const c10::cuda::CUDAGuard guard(x.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_instnorm_cl_fwd_launch(x.data_ptr(), y.data_ptr(),
                                 mean.data_ptr<float>(),
                                 rstd.data_ptr<float>(),
                                 partials.data_ptr<float>(), N, C, P,
                                 (float)eps, bf16 ? 1 : 0, deterministic,
                                 stream);
  return {y, mean, rstd};
}

torch::Tensor instnorm_cl_bwd(torch::Tensor x, torch::Tensor dy,
                              torch::Tensor mean, torch::Tensor rstd,
                              bool deterministic) {
  const bool bf16 = x.scalar_type() == torch::kBFloat16;
  const int N = x.size(0), C = x.size(1);
  const long P = (long)x.size(2) * x.size(3);
  auto dx = torch::empty(x.sizes(), x.options(),
                         torch::MemoryFormat::ChannelsLast);
  auto gmean = torch::empty_like(mean);
  auto gxmean = torch::empty_like(mean);
  auto partials = torch::empty({(long)flowhip_instnorm_partial_rows(N, C, P),
                                64},
                               x.options().dtype(torch::kFloat32));
  const c10::cuda::CUDAGuard guard(x.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_instnorm_cl_bwd_launch(x.data_ptr(), dy.data_ptr(),
                                 mean.data_ptr<float>(),
                                 rstd.data_ptr<float>(),
                                 gmean.data_ptr<float>(),
                                 gxmean.data_ptr<float>(),
                                 partials.data_ptr<float>(), dx.data_ptr(),
                                 N, C, P, bf16 ? 1 : 0, deterministic,
                                 stream);
  return dx;
}

std::vector<torch::Tensor> conf_pool_fwd(torch::Tensor data,
                                         torch::Tensor conf) {
  TORCH_CHECK(data.is_cuda() && data.is_contiguous() &&
              data.dtype() == torch::kFloat32);
  TORCH_CHECK(conf.is_cuda() && conf.is_contiguous() &&
              conf.sizes() == data.sizes());
  const long N = data.size(0), C = data.size(1);
  const int H = data.size(2), W = data.size(3);
  const int OH = H / 2, OW = W / 2;
  auto dds = torch::empty({N, C, (long)OH, (long)OW}, data.options());
  auto cds = torch::empty_like(dds);
  auto code = torch::empty({N, C, (long)OH, (long)OW},
                           data.options().dtype(torch::kUInt8));
  const c10::cuda::CUDAGuard guard(data.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_conf_pool_fwd_launch(data.data_ptr<float>(),
                               conf.data_ptr<float>(), dds.data_ptr<float>(),
                               cds.data_ptr<float>(),
                               code.data_ptr<unsigned char>(), dds.numel(),
                               H, W, OH, OW, stream);
  return {dds, cds, code};
}

std::vector<torch::Tensor> conf_pool_bwd(c10::optional<torch::Tensor> gdds,
                                         c10::optional<torch::Tensor> gcds,
                                         torch::Tensor code,
                                         std::vector<int64_t> in_shape) {
  TORCH_CHECK(gdds.has_value() || gcds.has_value());
  auto& any = gdds.has_value() ? gdds.value() : gcds.value();
  const int H = in_shape[2], W = in_shape[3];
  const int OH = code.size(2), OW = code.size(3);
  auto gdata = torch::empty(in_shape, any.options());
  auto gconf = torch::empty(in_shape, any.options());
  const c10::cuda::CUDAGuard guard(any.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_conf_pool_bwd_launch(
      gdds.has_value() ? gdds->data_ptr<float>() : nullptr,
      gcds.has_value() ? gcds->data_ptr<float>() : nullptr,
      code.data_ptr<unsigned char>(), gdata.data_ptr<float>(),
      gconf.data_ptr<float>(), gdata.numel(), H, W, OH, OW, stream);
  return {gdata, gconf};
}

torch::Tensor transpose_cast_bf16(torch::Tensor in) {
  const bool bf = in.dtype() == torch::kBFloat16;
  TORCH_CHECK(in.is_cuda() && in.dim() == 3 && in.is_contiguous() &&
              (bf || in.dtype() == torch::kFloat32));
  const int B = in.size(0), M = in.size(1), N = in.size(2);
  auto out = torch::empty({(long)B, (long)N, (long)M},
                          in.options().dtype(torch::kBFloat16));
  const c10::cuda::CUDAGuard guard(in.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_transpose_cast_launch(in.data_ptr(), out.data_ptr(), B, M,
                                N, bf ? 1 : 0, stream);
  return out;
}

static const void* cg_zero_page() {
  static void* p = nullptr;
  if (p == nullptr) {
    hipMalloc(&p, 256);
    hipMemset(p, 0, 256);
  }
  return p;
}

// x: (N, C, H, W) with channels-last-like strides (stride(1)==1); a
// channel-narrowed view is allowed (ld_x = stride at dim 3 >= C).
static void cg_check_x(const torch::Tensor& x, int& ld) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 &&
              x.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(x.stride(1) == 1, "conv_gemm: channels-last layout required");
  ld = (int)x.stride(3);
  TORCH_CHECK(ld >= x.size(1) && x.stride(2) == (long)ld * x.size(3) &&
              x.stride(0) == (long)ld * x.size(3) * x.size(2));
}

// The geometry of a same-padding conv over x (and the virtually
// concatenated x2) whose m axis walks N x OH x OW pixels of Cout channels.
static ConvGeom cg_geom(const torch::Tensor& x,
                        const c10::optional<torch::Tensor>& x2, int64_t Cout,
                        int64_t OH, int64_t OW, int64_t KH, int64_t KW,
                        int64_t sH, int64_t sW) {
  ConvGeom g{};
  cg_check_x(x, g.ld_x);
  g.srcH = x.size(2); g.srcW = x.size(3);
  g.C1 = g.Cin = x.size(1);
  if (x2.has_value()) {
    cg_check_x(x2.value(), g.ld_x2);
    TORCH_CHECK(x2->size(0) == x.size(0) && x2->size(2) == g.srcH &&
                x2->size(3) == g.srcW);
    g.Cin += (int)x2->size(1);
  }
  g.cpad = cg_cpad(g.Cin);
  g.Cout = (int)Cout; g.HH = (int)OH; g.WW = (int)OW;
  g.Mtot = x.size(0) * OH * OW;
  g.KH = (int)KH; g.KW = (int)KW; g.padH = g.KH / 2; g.padW = g.KW / 2;
  g.sH = (int)sH; g.sW = (int)sW;
  return g;
}

static const void* cg_ptr(const c10::optional<torch::Tensor>& t) {
  return t.has_value() ? t->data_ptr() : nullptr;
}

// FLOWHIP_CONV_FOLD=0 keeps every conv off the tap-folded path (A/B
// switch, default on): auto plans and the Python pack choice ask here.
static bool conv_fold_enabled() {
  const char* e = std::getenv("FLOWHIP_CONV_FOLD");
  return !(e != nullptr && e[0] == '0' && e[1] == '\0');
}

// fold: the folded forward layout (KH, O, 64) of conv_fold.h
torch::Tensor conv_gemm_pack(torch::Tensor w, bool flip, bool fold) {
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() &&
              w.scalar_type() == torch::kFloat32 && w.dim() == 4);
  const int O = w.size(0), I = w.size(1), KH = w.size(2), KW = w.size(3);
  TORCH_CHECK(!fold || (!flip && I <= 8 && KW <= 8),
              "conv_gemm_pack: a folded pack is a forward pack of at most 8 "
              "input channels and 8 taps per kernel row");
  const int R0 = flip ? I : O;
  const int cpad = cg_cpad(flip ? O : I);
  auto wpk = torch::empty({fold ? (long)KH : (long)KH * KW, (long)R0,
                           (long)cpad},
                          w.options().dtype(torch::kBFloat16));
  const c10::cuda::CUDAGuard guard(w.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_conv_gemm_pack_launch(w.data_ptr<float>(), wpk.data_ptr(),
                                wpk.numel(), O, I, KH, KW, cpad,
                                fold ? 2 : (flip ? 1 : 0), stream);
  return wpk;
}

std::vector<torch::Tensor> conv_gemm_fwd2(
    torch::Tensor x, c10::optional<torch::Tensor> x2, torch::Tensor wpk,
    c10::optional<torch::Tensor> bias, int64_t Cout, int64_t KH, int64_t KW,
    int64_t osplit, int64_t act, int64_t sH, int64_t sW, int64_t smode,
    int64_t outH, int64_t outW, bool fold) {
  TORCH_CHECK(wpk.is_cuda() && wpk.is_contiguous() &&
              wpk.scalar_type() == torch::kBFloat16 && wpk.dim() == 3);
  TORCH_CHECK(wpk.size(0) == (fold ? KH : KH * KW) && wpk.size(1) == Cout);
  TORCH_CHECK(smode >= 0 && smode <= 2 && sH >= 1 && sW >= 1);
  TORCH_CHECK(x.dim() == 4);
  // output spatial dims: same-pad for smode 0/1; smode 2 (strided
  // transposed conv, = backward-data of smode 1) takes them explicitly
  const long N = x.size(0);
  int64_t OH = x.size(2), OW = x.size(3);
  if (smode == 1) {
    OH = (OH + 2 * (KH / 2) - KH) / sH + 1;
    OW = (OW + 2 * (KW / 2) - KW) / sW + 1;
  } else if (smode == 2) {
    TORCH_CHECK(outH > 0 && outW > 0, "conv_gemm smode=2 needs outH/outW");
    OH = outH; OW = outW;
  }
  ConvGeom g = cg_geom(x, x2, Cout, OH, OW, KH, KW, sH, sW);
  TORCH_CHECK(!x2.has_value() || g.C1 % 64 == 0,
              "conv_gemm cat2: first input must be a "
              "multiple of 64 channels");
  g.cpad = wpk.size(2);
  if (smode == 0) g.sH = g.sW = 1;  // smode 0 ignores the stride arguments
  TORCH_CHECK(!fold || (smode <= 1 && wpk.size(2) == 64 &&
                        (osplit <= 0 || osplit >= Cout) &&
                        flowhip_conv_fold_envelope(g)),
              "conv_gemm: a folded pack on a conv outside the folded "
              "envelope (one source of 8 channels, KW <= 8, same padding, "
              "stride 1 or 2, direct)");
  const float* bptr = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_contiguous() &&
                bias->scalar_type() == torch::kFloat32 &&
                bias->numel() == Cout);
    bptr = bias->data_ptr<float>();
  }
  const c10::cuda::CUDAGuard guard(x.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  if (osplit <= 0 || osplit >= Cout) {
    auto out = torch::empty({N, Cout, OH, OW}, x.options(),
                            torch::MemoryFormat::ChannelsLast);
    flowhip_conv_gemm_fwd_launch(x.data_ptr(), cg_ptr(x2), wpk.data_ptr(),
                                 bptr, out.data_ptr(), nullptr,
                                 cg_zero_page(), g, (int)Cout, (int)act,
                                 (int)smode, stream, fold);
    return {out};
  }
  TORCH_CHECK(smode == 0, "conv_gemm: osplit only with smode 0");
  auto out = torch::empty({N, osplit, OH, OW}, x.options(),
                          torch::MemoryFormat::ChannelsLast);
  auto out2 = torch::empty({N, Cout - osplit, OH, OW}, x.options(),
                           torch::MemoryFormat::ChannelsLast);
  flowhip_conv_gemm_fwd_launch(x.data_ptr(), cg_ptr(x2), wpk.data_ptr(), bptr,
                               out.data_ptr(), out2.data_ptr(),
                               cg_zero_page(), g, (int)osplit, (int)act, 0,
                               stream);
  return {out, out2};
}

torch::Tensor conv_gemm_fwd(torch::Tensor x, torch::Tensor wpk,
                            c10::optional<torch::Tensor> bias, int64_t Cout,
                            int64_t KH, int64_t KW, int64_t act) {
  return conv_gemm_fwd2(x, c10::nullopt, wpk, bias, Cout, KH, KW, 0,
                        act, 1, 1, 0, 0, 0, false)[0];
}

// Weight gradient. The one-shot conv_gemm_wrw is the three steps below in
// one call: plan -> partials (overwrite) -> finish. Callers that sum the
// gradients of several calls (same weights, same shapes) run the steps
// themselves: plan -> partials (accumulate) x K -> finish.
static ConvGeom cg_wrw_geom(const torch::Tensor& dy, const torch::Tensor& x,
                            const c10::optional<torch::Tensor>& x2,
                            int64_t KH, int64_t KW, int64_t sH, int64_t sW) {
  TORCH_CHECK(dy.is_cuda() && dy.dim() == 4 &&
              dy.scalar_type() == torch::kBFloat16 && dy.stride(1) == 1 &&
              dy.stride(3) == dy.size(1),
              "conv_gemm_wrw: dy must be channels-last contiguous");
  TORCH_CHECK(x.dim() == 4 && dy.size(0) == x.size(0));
  return cg_geom(x, x2, dy.size(1), dy.size(2), dy.size(3), KH, KW, sH, sW);
}

// path (generic per-tap | halo-staged | folded) and its split-M chunk
// count. The folded decision is taken here, before the plan of conv_gemm.h:
// auto takes path 2 inside its envelope. *form: the folded kernel's ky form
// (ky_form: -1 its rule, 0 | 1 forced), 0 on the other paths.
static int cg_wrw_plan(const ConvGeom& g, int64_t algo, int64_t nchunk_req,
                       int64_t ky_form, int* nchunk, int* form) {
  TORCH_CHECK(algo >= -1 && algo <= 2,
              "conv_gemm_wrw: algo must be -1, 0, 1, 2");
  TORCH_CHECK(ky_form >= -1 && ky_form <= 1,
              "conv_gemm_wrw: ky_form must be -1, 0, 1");
  *form = 0;
  const bool in_fold = flowhip_conv_fold_wrw_envelope(g);
  TORCH_CHECK(algo != 2 || in_fold,
              "conv_gemm_wrw: algo=2 (folded) forced on a shape outside its "
              "envelope (one source of 8 channels, KW <= 8, same padding, "
              "stride 1 or 2, Cout % 8 == 0)");
  if (algo == 2 || (algo == -1 && in_fold && conv_fold_enabled())) {
    *form = flowhip_conv_fold_wrw_plan(g, (int)ky_form, (int)nchunk_req,
                                       nchunk);
    TORCH_CHECK(*form >= 0,
                "conv_gemm_wrw: ky_form=1 needs KH <= ", CF_MAXKY);
    return 2;
  }
  const int path =
      flowhip_conv_gemm_wrw_plan(g, (int)algo, (int)nchunk_req, nchunk);
  TORCH_CHECK(path >= 0,
              "conv_gemm_wrw: algo=1 (halo) forced on a shape outside its "
              "envelope (stride 1, same padding, 3x3 / 1x5 / 5x1)");
  return path;
}

std::vector<torch::Tensor> conv_gemm_wrw(torch::Tensor dy, torch::Tensor x,
                                         c10::optional<torch::Tensor> x2,
                                         int64_t KH, int64_t KW, int64_t sH,
                                         int64_t sW, bool want_bias,
                                         int64_t algo, int64_t nchunk_req,
                                         int64_t ky_form) {
  const ConvGeom g = cg_wrw_geom(dy, x, x2, KH, KW, sH, sW);
  int nchunk = 1, form = 0;
  const int path = cg_wrw_plan(g, algo, nchunk_req, ky_form, &nchunk, &form);
  // every slot the reduce reads is written by the partials launch, and
  // dw / dbias fully by the reduce: no zero-fill
  const auto f32 = x.options().dtype(torch::kFloat32);
  auto partials = torch::empty(
      {path == 2 ? cf_buffer_numel(g, nchunk, want_bias)
                 : g.buffer_numel(nchunk, want_bias)}, f32);
  auto dw = torch::empty({(long)g.Cout, (long)g.Cin, KH, KW}, f32);
  torch::Tensor dbias;
  if (want_bias) dbias = torch::empty({(long)g.Cout}, f32);
  const c10::cuda::CUDAGuard guard(x.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  if (path == 2) {
    flowhip_conv_fold_wrw_partials_launch(
        dy.data_ptr(), x.data_ptr(), partials.data_ptr<float>(), want_bias,
        cg_zero_page(), g, nchunk, form, false, stream);
    flowhip_conv_fold_wrw_finish_launch(
        partials.data_ptr<float>(), dw.data_ptr<float>(),
        want_bias ? dbias.data_ptr<float>() : nullptr, g, nchunk, false,
        stream);
    return {dw, dbias};
  }
  const bool launched = flowhip_conv_gemm_wrw_partials_launch(
      dy.data_ptr(), x.data_ptr(), cg_ptr(x2), partials.data_ptr<float>(),
      want_bias, cg_zero_page(), g, nchunk, path, false, stream);
  TORCH_CHECK(launched,
              "conv_gemm_wrw: the halo kernel refused a planned shape");
  flowhip_conv_gemm_wrw_finish_launch(
      partials.data_ptr<float>(), dw.data_ptr<float>(),
      want_bias ? dbias.data_ptr<float>() : nullptr, g, nchunk, false,
      stream);
  return {dw, dbias};
}

// -> (path, nchunk, buffer elements, accumulate). The buffer size includes
// the bias partials when want_bias. accumulate: 1 where calls that share a
// weight should sum their partials in one buffer, 0 where they should run
// one-shot partials and add each finish to a running dW.
std::vector<int64_t> conv_gemm_wrw_plan(torch::Tensor dy, torch::Tensor x,
                                        c10::optional<torch::Tensor> x2,
                                        int64_t KH, int64_t KW, int64_t sH,
                                        int64_t sW, bool want_bias,
                                        int64_t algo, int64_t nchunk_req,
                                        int64_t ky_form) {
  const ConvGeom g = cg_wrw_geom(dy, x, x2, KH, KW, sH, sW);
  int nchunk = 1, form = 0;
  const int path = cg_wrw_plan(g, algo, nchunk_req, ky_form, &nchunk, &form);
  if (path == 2)
    return {path, nchunk, cf_buffer_numel(g, nchunk, want_bias),
            flowhip_conv_fold_accumulate_wins() ? 1 : 0};
  return {path, nchunk, g.buffer_numel(nchunk, want_bias),
          flowhip_conv_gemm_wrw_accumulate_wins(path) ? 1 : 0};
}

// One partials launch into the caller's buffer; no reduce. algo / nchunk:
// what conv_gemm_wrw_plan returned for these shapes (checked again here,
// because a wrong pair would size the grid past the buffer).
void conv_gemm_wrw_partials(torch::Tensor dy, torch::Tensor x,
                            c10::optional<torch::Tensor> x2,
                            torch::Tensor partials, int64_t KH, int64_t KW,
                            int64_t sH, int64_t sW, bool want_bias,
                            bool accumulate, int64_t algo, int64_t nchunk,
                            int64_t ky_form) {
  const ConvGeom g = cg_wrw_geom(dy, x, x2, KH, KW, sH, sW);
  TORCH_CHECK(algo >= 0 && algo <= 2,
              "conv_gemm_wrw_partials: algo must be a planned path (0 | 1 | "
              "2)");
  TORCH_CHECK(nchunk >= 1, "conv_gemm_wrw_partials: nchunk must be planned");
  int planned = 0, form = 0;
  const int path = cg_wrw_plan(g, algo, nchunk, ky_form, &planned, &form);
  TORCH_CHECK(path == algo && planned == nchunk,
              "conv_gemm_wrw_partials: (algo, nchunk) is not a plan for "
              "these shapes");
  TORCH_CHECK(partials.is_cuda() && partials.is_contiguous() &&
              partials.scalar_type() == torch::kFloat32 &&
              partials.device() == x.device() &&
              partials.numel() ==
                  (path == 2 ? cf_buffer_numel(g, (int)nchunk, want_bias)
                             : g.buffer_numel((int)nchunk, want_bias)),
              "conv_gemm_wrw_partials: buffer does not match the plan");
  const c10::cuda::CUDAGuard guard(x.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  if (path == 2) {
    flowhip_conv_fold_wrw_partials_launch(
        dy.data_ptr(), x.data_ptr(), partials.data_ptr<float>(), want_bias,
        cg_zero_page(), g, (int)nchunk, form, accumulate, stream);
    return;
  }
  const bool launched = flowhip_conv_gemm_wrw_partials_launch(
      dy.data_ptr(), x.data_ptr(), cg_ptr(x2), partials.data_ptr<float>(),
      want_bias, cg_zero_page(), g, (int)nchunk, (int)algo, accumulate,
      stream);
  TORCH_CHECK(launched,
              "conv_gemm_wrw: the halo kernel refused a planned shape");
}

// Reduce a partials buffer to [dw (Cout, Cin, KH, KW), dbias (Cout)]. With
// dw_into (and dbias_into when want_bias) the sums are added to those
// tensors in place and they are returned.
std::vector<torch::Tensor> conv_gemm_wrw_finish(
    torch::Tensor partials, int64_t Cout, int64_t Cin, int64_t KH,
    int64_t KW, bool want_bias, int64_t nchunk,
    c10::optional<torch::Tensor> dw_into,
    c10::optional<torch::Tensor> dbias_into, int64_t path) {
  TORCH_CHECK(Cout >= 1 && Cin >= 1 && KH >= 1 && KW >= 1 && nchunk >= 1);
  TORCH_CHECK(path >= 0 && path <= 2, "conv_gemm_wrw_finish: path 0 | 1 | 2");
  const bool fold = path == 2;  // the folded buffer layout (conv_fold.h)
  TORCH_CHECK(!fold || (Cin == 8 && KW <= 8),
              "conv_gemm_wrw_finish: path 2 is the folded layout (Cin 8, "
              "KW <= 8)");
  ConvGeom g{};  // the reduce needs the buffer layout only
  g.Cout = (int)Cout; g.Cin = (int)Cin; g.cpad = cg_cpad(g.Cin);
  g.KH = (int)KH; g.KW = (int)KW;
  TORCH_CHECK(partials.is_cuda() && partials.is_contiguous() &&
              partials.scalar_type() == torch::kFloat32 &&
              partials.numel() ==
                  (fold ? cf_buffer_numel(g, (int)nchunk, want_bias)
                        : g.buffer_numel((int)nchunk, want_bias)),
              "conv_gemm_wrw_finish: buffer does not match the shapes");
  const bool accumulate = dw_into.has_value();
  TORCH_CHECK(dbias_into.has_value() == (accumulate && want_bias),
              "conv_gemm_wrw_finish: dw_into and dbias_into go together");
  torch::Tensor dw, dbias;
  if (accumulate) {
    dw = dw_into.value();
    TORCH_CHECK(dw.is_contiguous() && dw.device() == partials.device() &&
                dw.scalar_type() == torch::kFloat32 &&
                dw.sizes() == at::IntArrayRef({Cout, Cin, KH, KW}),
                "conv_gemm_wrw_finish: dw_into does not match the shapes");
    if (want_bias) {
      dbias = dbias_into.value();
      TORCH_CHECK(dbias.is_contiguous() &&
                  dbias.device() == partials.device() &&
                  dbias.scalar_type() == torch::kFloat32 &&
                  dbias.dim() == 1 && dbias.size(0) == Cout,
                  "conv_gemm_wrw_finish: dbias_into does not match");
    }
  } else {
    dw = torch::empty({Cout, Cin, KH, KW}, partials.options());
    if (want_bias) dbias = torch::empty({Cout}, partials.options());
  }
  const c10::cuda::CUDAGuard guard(partials.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  (fold ? flowhip_conv_fold_wrw_finish_launch
        : flowhip_conv_gemm_wrw_finish_launch)(
      partials.data_ptr<float>(), dw.data_ptr<float>(),
      want_bias ? dbias.data_ptr<float>() : nullptr, g, (int)nchunk,
      accumulate, stream);
  return {dw, dbias};
}

torch::Tensor col_sum_bf16(torch::Tensor dy, bool deterministic) {
  TORCH_CHECK(dy.is_cuda() && dy.dim() == 4 &&
              dy.scalar_type() == torch::kBFloat16 && dy.stride(1) == 1 &&
              dy.stride(3) == dy.size(1));
  const int C = dy.size(1);
  const long M = dy.numel() / C;
  const int nchunk = (int)((M + 255) / 256);  // must cover ALL rows (kernel bounds come from the chunk index)
  const auto f32 = dy.options().dtype(torch::kFloat32);
  // deterministic: one row per chunk, added in chunk order by a finish
  // kernel; nothing accumulates in place, so nothing is zero-filled
  auto out = deterministic ? torch::empty({(long)C}, f32)
                           : torch::zeros({(long)C}, f32);
  torch::Tensor partials;
  if (deterministic) partials = torch::empty({(long)nchunk, (long)C}, f32);
  const c10::cuda::CUDAGuard guard(dy.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  bool ok = flowhip_col_sum_launch(
      dy.data_ptr(), out.data_ptr<float>(),
      deterministic ? partials.data_ptr<float>() : nullptr, M, C, nchunk,
      stream);
  TORCH_CHECK(ok, "col_sum_bf16: C must be a multiple of 8");
  return out;
}

torch::Tensor plane_sum_nchw(torch::Tensor x, c10::optional<torch::Tensor> y) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.is_contiguous() &&
              x.scalar_type() == torch::kFloat32);
  const float* yp = nullptr;
  if (y.has_value()) {
    TORCH_CHECK(y->sizes() == x.sizes() && y->is_contiguous() &&
                y->scalar_type() == torch::kFloat32);
    yp = y->data_ptr<float>();
  }
  const int B = x.size(0), C = x.size(1);
  const long P = (long)x.size(2) * x.size(3);
  auto out = torch::empty({(long)C}, x.options());
  auto partials = torch::empty(
      {(long)C, (long)B * flowhip_plane_dot_sum_pchunks(P, B, C)},
      x.options());
  const c10::cuda::CUDAGuard guard(x.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_plane_dot_sum_launch(x.data_ptr<float>(), yp,
                               partials.data_ptr<float>(),
                               out.data_ptr<float>(), P, B, C, stream);
  return out;
}

torch::Tensor frozen_bn_apply(torch::Tensor x, torch::Tensor s,
                              c10::optional<torch::Tensor> t) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 &&
              x.scalar_type() == torch::kBFloat16 && x.stride(1) == 1 &&
              x.stride(3) == x.size(1) && x.size(1) % 8 == 0);
  TORCH_CHECK(s.is_contiguous() && s.scalar_type() == torch::kFloat32 &&
              s.numel() == x.size(1));
  const float* tp = nullptr;
  if (t.has_value()) {
    TORCH_CHECK(t->is_contiguous() && t->scalar_type() == torch::kFloat32 &&
                t->numel() == x.size(1));
    tp = t->data_ptr<float>();
  }
  auto y = torch::empty_like(x);
  const c10::cuda::CUDAGuard guard(x.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_frozen_bn_apply_launch(x.data_ptr(), y.data_ptr(),
                                 s.data_ptr<float>(), tp,
                                 x.numel() / x.size(1), (int)x.size(1),
                                 stream);
  return y;
}

torch::Tensor col_sum2_bf16(torch::Tensor g, torch::Tensor x,
                            bool deterministic) {
  TORCH_CHECK(g.is_cuda() && g.dim() == 4 &&
              g.scalar_type() == torch::kBFloat16 && g.stride(1) == 1 &&
              g.stride(3) == g.size(1));
  TORCH_CHECK(x.sizes() == g.sizes() && x.strides() == g.strides() &&
              x.scalar_type() == torch::kBFloat16);
  const int C = g.size(1);
  const long M = g.numel() / C;
  const int nchunk = (int)((M + 255) / 256);
  const auto f32 = g.options().dtype(torch::kFloat32);
  auto out = deterministic ? torch::empty({2, (long)C}, f32)
                           : torch::zeros({2, (long)C}, f32);
  torch::Tensor partials;
  if (deterministic)
    partials = torch::empty({(long)nchunk, 2, (long)C}, f32);
  const c10::cuda::CUDAGuard guard(g.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  bool ok = flowhip_col_sum2_launch(
      g.data_ptr(), x.data_ptr(), out.data_ptr<float>(),
      deterministic ? partials.data_ptr<float>() : nullptr, M, C, nchunk,
      stream);
  TORCH_CHECK(ok, "col_sum2_bf16: C must be a multiple of 8");
  return out;
}

torch::Tensor up2x_cat_fwd(torch::Tensor low, torch::Tensor skip) {
  TORCH_CHECK(low.is_cuda() && low.is_contiguous() &&
              low.dtype() == torch::kFloat32);
  TORCH_CHECK(skip.is_cuda() && skip.is_contiguous() &&
              skip.sizes()[0] == low.sizes()[0]);
  const long N = skip.size(0), C1 = low.size(1), C2 = skip.size(1);
  const int H = skip.size(2), W = skip.size(3);
  auto out = torch::empty({N, C1 + C2, (long)H, (long)W}, low.options());
  const c10::cuda::CUDAGuard guard(low.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_up2x_cat_fwd_launch(low.data_ptr<float>(), skip.data_ptr<float>(),
                              out.data_ptr<float>(), out.numel(), (int)C1,
                              (int)C2, H, W, stream);
  return out;
}

torch::Tensor area_up2x_fwd(torch::Tensor in) {
  TORCH_CHECK(in.is_cuda() && in.is_contiguous() && in.dim() == 4 &&
              in.dtype() == torch::kFloat32);
  const long N = in.size(0), C = in.size(1);
  const int H = in.size(2), W = in.size(3);
  auto out = torch::empty({N, C, (long)2 * H, (long)2 * W}, in.options());
  const c10::cuda::CUDAGuard guard(in.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_area_up2x_fwd_launch(in.data_ptr<float>(), out.data_ptr<float>(),
                               out.numel(), H, W, stream);
  return out;
}

torch::Tensor area_up2x_bwd(torch::Tensor gout) {
  auto g = gout.contiguous();
  const long N = g.size(0), C = g.size(1);
  const int H = g.size(2) / 2, W = g.size(3) / 2;
  auto gin = torch::empty({N, C, (long)H, (long)W}, g.options());
  const c10::cuda::CUDAGuard guard(g.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_area_up2x_bwd_launch(g.data_ptr<float>(), gin.data_ptr<float>(),
                               gin.numel(), H, W, stream);
  return gin;
}

torch::Tensor packernel_fwd(torch::Tensor f, int64_t K, int64_t dil,
                            bool normalize) {
  TORCH_CHECK(f.is_cuda() && f.is_contiguous() && f.dim() == 4 &&
              f.dtype() == torch::kFloat32);
  const int B = f.size(0), C = f.size(1), H = f.size(2), W = f.size(3);
  auto k = torch::empty({(long)B, K * K, (long)H, (long)W}, f.options());
  const c10::cuda::CUDAGuard guard(f.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  bool ok = flowhip_packernel_fwd_launch(f.data_ptr<float>(),
                                         k.data_ptr<float>(), B, C, H, W,
                                         (int)K, (int)dil, normalize ? 1 : 0,
                                         stream);
  TORCH_CHECK(ok, "packernel: unsupported K");
  return k;
}

torch::Tensor packernel_bwd(torch::Tensor f, torch::Tensor k,
                            torch::Tensor dk, int64_t K, int64_t dil,
                            bool normalize) {
  const int B = f.size(0), C = f.size(1), H = f.size(2), W = f.size(3);
  auto df = torch::empty_like(f);
  const c10::cuda::CUDAGuard guard(f.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  bool ok = flowhip_packernel_bwd_launch(
      f.data_ptr<float>(), k.data_ptr<float>(), dk.data_ptr<float>(),
      df.data_ptr<float>(), B, C, H, W, (int)K, (int)dil, normalize ? 1 : 0,
      stream);
  TORCH_CHECK(ok);
  return df;
}

torch::Tensor pacconv_fwd(torch::Tensor x, torch::Tensor kr,
                          torch::Tensor w, c10::optional<torch::Tensor> bias,
                          int64_t pH, int64_t pW, int64_t dil, bool shared) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() &&
              x.dtype() == torch::kFloat32);
  TORCH_CHECK(kr.is_contiguous() && w.is_contiguous());
  const int B = x.size(0), Ci = x.size(1), H = x.size(2), W = x.size(3);
  const int K = w.size(-1);
  const int Co = shared ? Ci : (int)w.size(0);
  const int OH = H + 2 * (int)pH - ((K - 1) * (int)dil);
  const int OW = W + 2 * (int)pW - ((K - 1) * (int)dil);
  TORCH_CHECK(kr.size(-2) == OH && kr.size(-1) == OW,
              "pacconv: kernel grid must match the output grid");
  auto out = torch::empty({(long)B, (long)Co, (long)OH, (long)OW},
                          x.options());
  const c10::cuda::CUDAGuard guard(x.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  bool ok = flowhip_pacconv_fwd_launch(
      x.data_ptr<float>(), kr.data_ptr<float>(), w.data_ptr<float>(),
      bias.has_value() ? bias->data_ptr<float>() : nullptr,
      out.data_ptr<float>(), B, Ci, Co, H, W, OH, OW, (int)pH, (int)pW, K,
      (int)dil, shared ? 1 : 0, stream);
  TORCH_CHECK(ok, "pacconv: unsupported K");
  return out;
}

std::vector<torch::Tensor> pacconv_bwd(torch::Tensor dy, torch::Tensor x,
                                       torch::Tensor kr, torch::Tensor w,
                                       int64_t pH, int64_t pW, int64_t dil,
                                       bool shared) {
  const int B = x.size(0), Ci = x.size(1), H = x.size(2), W = x.size(3);
  const int K = w.size(-1);
  const int Co = shared ? Ci : (int)w.size(0);
  const int OH = dy.size(2), OW = dy.size(3);
  const int K2 = K * K;
  const int nw = shared ? K2 : Co * Ci * K2;
  TORCH_CHECK((long)nw * 4 <= 65536, "pacconv dw: weight too large for the "
              "LDS-accumulated backward");
  const int nchunk = 512;
  auto dx = torch::empty_like(x);
  auto dk = torch::empty_like(kr);
  auto partials = torch::empty({(long)nchunk * nw},
                               x.options().dtype(torch::kFloat32));
  auto dw = torch::empty_like(w);
  const c10::cuda::CUDAGuard guard(x.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  bool ok = flowhip_pacconv_bwd_launch(
      dy.data_ptr<float>(), x.data_ptr<float>(), kr.data_ptr<float>(),
      w.data_ptr<float>(), dx.data_ptr<float>(), dk.data_ptr<float>(),
      partials.data_ptr<float>(), dw.data_ptr<float>(), nchunk, B, Ci, Co, H,
      W, OH, OW, (int)pH, (int)pW, K, (int)dil, shared ? 1 : 0, stream);
  TORCH_CHECK(ok);
  return {dx, dk, dw};
}

// kr: (B, KCH, K2, OH, OW) fp32; x: (B, C, H, W) fp32
torch::Tensor pacpool_fwd(torch::Tensor x, torch::Tensor kr, int64_t K,
                          int64_t sH, int64_t sW, int64_t pH, int64_t pW,
                          int64_t dil) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() &&
              x.scalar_type() == torch::kFloat32);
  TORCH_CHECK(kr.is_cuda() && kr.is_contiguous() && kr.dim() == 5 &&
              kr.size(2) == K * K);
  const int B = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int KCH = kr.size(1), OH = kr.size(3), OW = kr.size(4);
  TORCH_CHECK(KCH == 1 || KCH == C);
  auto out = torch::empty({(long)B, (long)C, (long)OH, (long)OW},
                          x.options());
  const c10::cuda::CUDAGuard guard(x.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_pacpool_fwd_launch(x.data_ptr<float>(), kr.data_ptr<float>(),
                             out.data_ptr<float>(), B, C, KCH, H, W, OH, OW,
                             (int)K, (int)sH, (int)sW, (int)pH, (int)pW,
                             (int)dil, stream);
  return out;
}

std::vector<torch::Tensor> pacpool_bwd(torch::Tensor dy, torch::Tensor x,
                                       torch::Tensor kr, int64_t K,
                                       int64_t sH, int64_t sW, int64_t pH,
                                       int64_t pW, int64_t dil) {
  const int B = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int KCH = kr.size(1), OH = kr.size(3), OW = kr.size(4);
  auto dx = torch::zeros_like(x);
  auto dk = torch::empty_like(kr);
  const c10::cuda::CUDAGuard guard(x.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
  flowhip_pacpool_bwd_launch(dy.contiguous().data_ptr<float>(),
                             x.data_ptr<float>(), kr.data_ptr<float>(),
                             dx.data_ptr<float>(), dk.data_ptr<float>(), B,
                             C, KCH, H, W, OH, OW, (int)K, (int)sH, (int)sW,
                             (int)pH, (int)pW, (int)dil, stream);
  return {dx, dk};
}

}  // namespace

// Whole normalized-convolution backward of one layer ->
// {ddata, dconf, dweight, dbias (empty without bias)}.
// algo 1: the fused kernel of nconv_bwd_fused.hip (one pass + reduce);
// algo 0: the split path (prep, bwd-data, wrw + reduce, plane sums and the
// torch glue between them); algo -1: automatic, which is fused — the two
// paths share one envelope. gout or gcout may be absent (treated as zeros),
// not both.
std::vector<torch::Tensor> nconv_bwd_fused(
    c10::optional<torch::Tensor> gout, c10::optional<torch::Tensor> gcout,
    torch::Tensor out, torch::Tensor cout, torch::Tensor data,
    torch::Tensor conf, torch::Tensor weight,
    c10::optional<torch::Tensor> bias, double eps, int64_t algo,
    int64_t strip) {
  const char* who = "nconv_bwd_fused";
  TORCH_CHECK(algo >= -1 && algo <= 1, "nconv_bwd_fused: algo must be -1, 0, 1");
  TORCH_CHECK(gout.has_value() || gcout.has_value(),
              "nconv_bwd_fused: no upstream gradient");
  const NConvGeom g = nconv_geom(who, data, weight);
  nconv_check_planes(who, g, conf, g.Ci);
  nconv_check_planes(who, g, out, g.Co);
  nconv_check_planes(who, g, cout, g.Co);
  if (gout.has_value()) nconv_check_planes(who, g, *gout, g.Co);
  if (gcout.has_value()) nconv_check_planes(who, g, *gcout, g.Co);
  const float* bptr = nconv_bias_ptr(who, g, bias);

  const c10::cuda::CUDAGuard guard(data.device());
  if (algo != 0) {
    int st = (int)strip;
    const int nblocks = flowhip_nconv_bwd_fused_plan(g, &st);
    auto ddata = torch::empty_like(data);
    auto dconf = torch::empty_like(conf);
    auto dweight = torch::empty_like(weight);
    auto dbias = torch::empty({bias.has_value() ? (long)g.Co : 0L},
                              data.options());
    auto partials = torch::empty(
        {nblocks, (long)flowhip_nconv_bwd_fused_ncol(g)}, data.options());
    hipStream_t stream = at::cuda::getCurrentCUDAStream().stream();
    const bool ok = flowhip_nconv_bwd_fused_launch(
        gout.has_value() ? gout->data_ptr<float>() : nullptr,
        gcout.has_value() ? gcout->data_ptr<float>() : nullptr,
        out.data_ptr<float>(), cout.data_ptr<float>(),
        data.data_ptr<float>(), conf.data_ptr<float>(),
        weight.data_ptr<float>(), bptr, ddata.data_ptr<float>(),
        dconf.data_ptr<float>(), partials.data_ptr<float>(),
        dweight.data_ptr<float>(),
        bias.has_value() ? dbias.data_ptr<float>() : nullptr, g, st,
        (float)eps, stream);
    TORCH_CHECK(ok, "nconv_bwd_fused: launch refused a checked geometry");
    return {ddata, dconf, dweight, dbias};
  }

  // split path: the kernels the fused one replaced, and their torch glue
  auto s = weight.sum(at::IntArrayRef({1, 2, 3})).contiguous();
  auto go = gout.has_value() ? *gout : torch::zeros_like(out);
  auto pre = nconv_bwd_prep(go, gcout, out, cout, s, bias, eps);
  auto r = nconv_bwd(pre[0], pre[1], data, conf, weight);
  auto dweight = r[2];
  if (gcout.has_value()) {
    // cout = denom / s depends on s = sum(w) per out channel
    auto ds = -plane_sum_nchw(cout, *gcout) / s;
    dweight = dweight + ds.view({-1, 1, 1, 1});
  }
  auto dbias = bias.has_value() ? plane_sum_nchw(go, c10::nullopt)
                                : torch::empty({0}, data.options());
  return {r[0], r[1], dweight, dbias};
}

bool nconv_supported(int64_t Ci, int64_t Co, int64_t K) {
  return flowhip_nconv_supported((int)Ci, (int)Co, (int)K);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "flowhip gfx950 HIP kernels";
  m.def("bgemm_nt", &bgemm_nt,
        "C[b] = alpha * A[b] (M,K) @ B[b] (N,K)^T, bf16 in / fp32|bf16 out",
        py::arg("a"), py::arg("b"), py::arg("alpha"),
        py::arg("out_bf16") = false);
  m.def("corr_lookup_fwd", &corr_lookup_fwd,
        "fused multi-level correlation window lookup (fp32/bf16 levels)");
  m.def("alt_corr_lookup_fwd", &alt_corr_lookup_fwd,
        "on-demand correlation window lookup from feature maps");
  m.def("alt_corr_supported", &alt_corr_supported,
        "alt_corr_lookup_fwd envelope (D, radius, levels)");
  m.def("alt_corr_lookup_bwd", &alt_corr_lookup_bwd,
        "backward of alt_corr_lookup_fwd: (df1_rows | None, df2 | None)",
        py::arg("grad"), py::arg("f1_rows"), py::arg("levels"),
        py::arg("coords"), py::arg("radius"), py::arg("channels_last"),
        py::arg("need_f1") = true, py::arg("need_f2") = true,
        py::arg("algo") = "auto");
  m.def("corr_lookup_bwd", &corr_lookup_bwd,
        "backward of corr_lookup_fwd (pyramid grads; accumulates into "
        "`prev` when the pyramid is iteration-chained)",
        py::arg("gout"), py::arg("coords"), py::arg("radius"),
        py::arg("level_shapes"), py::arg("channels_last"),
        py::arg("levels_bf16") = false,
        py::arg("prev") = py::none());
  m.def("corr_pyramid_fits", &corr_pyramid_fits,
        "does the fused pyramid-build kernel support this map size/dtype");
  m.def("packernel_fwd", &packernel_fwd, "PAC gaussian adapting kernel");
  m.def("packernel_bwd", &packernel_bwd, "backward of packernel_fwd");
  m.def("pacconv_fwd", &pacconv_fwd, "pixel-adaptive convolution forward");
  m.def("pacconv_bwd", &pacconv_bwd, "pixel-adaptive conv backward (dx,dk,dw)");
  m.def("pacpool_fwd", &pacpool_fwd, "pixel-adaptive pooling forward");
  m.def("pacpool_bwd", &pacpool_bwd,
        "pixel-adaptive pooling backward (dx via atomic scatter, dk)");
  m.def("corr_pyramid_fwd", &corr_pyramid_fwd,
        "fused avg-pool pyramid build (levels 1..n-1)");
  m.def("corr_pyramid_bwd", &corr_pyramid_bwd,
        "fused pyramid backward combine -> dcorr");
  m.def("convex_up_fwd", &convex_up_fwd, "fused convex-combination upsample");
  m.def("convex_up_bwd", &convex_up_bwd, "backward of convex_up_fwd",
        py::arg("gout"), py::arg("flow"), py::arg("mask"), py::arg("factor"),
        py::arg("deterministic") = false);
  m.def("nconv_fwd", &nconv_fwd,
        "fused normalized convolution forward (out, cout)");
  m.def("plane_sum_nchw", &plane_sum_nchw,
        "out[c] = sum_{b,h,w} x (or x*y), NCHW fp32",
        py::arg("x"), py::arg("y") = py::none());
  m.def("frozen_bn_apply", &frozen_bn_apply,
        "y = bf16(fp32(x)*s + t) per channel, channels-last");
  m.def("col_sum2_bf16", &col_sum2_bf16,
        "(sum_m g, sum_m g*x) per channel in one pass (frozen-BN backward)",
        py::arg("g"), py::arg("x"), py::arg("deterministic") = false);
  m.def("col_sum_bf16", &col_sum_bf16,
        "(N,C,H,W) channels-last bf16 -> (C) fp32 bias-grad column sum",
        py::arg("dy"), py::arg("deterministic") = false);
  m.def("up2x_cat_fwd", &up2x_cat_fwd,
        "fused nearest-2x upsample + channel concat");
  m.def("area_up2x_fwd", &area_up2x_fwd, "exact-2x area upsample");
  m.def("area_up2x_bwd", &area_up2x_bwd, "backward of area_up2x");
  m.def("conf_pool_fwd", &conf_pool_fwd,
        "confidence-based 2x pooling forward (data_ds, conf_ds, argmax code)");
  m.def("conf_pool_bwd", &conf_pool_bwd, "backward of conf_pool");
  m.def("transpose_cast_bf16", &transpose_cast_bf16,
        "(B,M,N) fp32 -> (B,N,M) bf16 tiled transpose");
  m.def("conv_gemm_pack", &conv_gemm_pack,
        "one-kernel conv weight packing (fwd, flipped-bwd or folded fwd "
        "layout)",
        py::arg("w"), py::arg("flip"), py::arg("fold") = false);
  m.def("conv_fold_enabled", &conv_fold_enabled,
        "false with FLOWHIP_CONV_FOLD=0: no conv takes the folded path "
        "unless forced");
  m.def("conv_gemm_fwd", &conv_gemm_fwd,
        "implicit-GEMM NHWC bf16 conv forward (also bwd-data with flipped "
        "packed weights)");
  m.def("conv_gemm_fwd2", &conv_gemm_fwd2,
        "conv forward over a virtually-concatenated pair of inputs and/or "
        "with a split output (bwd-data of a cat input); smode 1 = strided "
        "direct conv, smode 2 = strided transposed conv (bwd-data)",
        py::arg("x"), py::arg("x2"), py::arg("wpk"), py::arg("bias"),
        py::arg("Cout"), py::arg("KH"), py::arg("KW"), py::arg("osplit"),
        py::arg("act"), py::arg("sH") = 1, py::arg("sW") = 1,
        py::arg("smode") = 0, py::arg("outH") = 0, py::arg("outW") = 0,
        py::arg("fold") = false);
  m.def("conv_gemm_wrw", &conv_gemm_wrw,
        "implicit-GEMM conv weight gradient (split-M + reduce); returns "
        "[dw, dbias] — dbias undefined unless want_bias. algo: -1 auto, "
        "0 generic per-tap kernel, 1 halo-staged kernel, 2 folded kernel "
        "(ky_form: -1 its rule, 0 ky in the grid, 1 ky looped); nchunk: 0 "
        "auto",
        py::arg("dy"), py::arg("x"), py::arg("x2"), py::arg("KH"),
        py::arg("KW"), py::arg("sH") = 1, py::arg("sW") = 1,
        py::arg("want_bias") = false, py::arg("algo") = -1,
        py::arg("nchunk") = 0, py::arg("ky_form") = -1);
  m.def("conv_gemm_wrw_plan", &conv_gemm_wrw_plan,
        "weight-gradient plan for these shapes: [path, nchunk, partials "
        "buffer elements, accumulate (1: sum shared calls in the buffer)]",
        py::arg("dy"), py::arg("x"), py::arg("x2"), py::arg("KH"),
        py::arg("KW"), py::arg("sH") = 1, py::arg("sW") = 1,
        py::arg("want_bias") = false, py::arg("algo") = -1,
        py::arg("nchunk") = 0, py::arg("ky_form") = -1);
  m.def("conv_gemm_wrw_partials", &conv_gemm_wrw_partials,
        "one split-M partials launch into a caller-supplied buffer, no "
        "reduce; accumulate adds to the buffer instead of overwriting it",
        py::arg("dy"), py::arg("x"), py::arg("x2"), py::arg("partials"),
        py::arg("KH"), py::arg("KW"), py::arg("sH"), py::arg("sW"),
        py::arg("want_bias"), py::arg("accumulate"), py::arg("algo"),
        py::arg("nchunk"), py::arg("ky_form") = -1);
  m.def("conv_gemm_wrw_finish", &conv_gemm_wrw_finish,
        "reduce a partials buffer over its chunks; returns [dw, dbias], "
        "added in place to dw_into / dbias_into when given",
        py::arg("partials"), py::arg("Cout"), py::arg("Cin"), py::arg("KH"),
        py::arg("KW"), py::arg("want_bias"), py::arg("nchunk"),
        py::arg("dw_into") = py::none(), py::arg("dbias_into") = py::none(),
        py::arg("path") = 0);
  m.def("instnorm_cl_fwd", &instnorm_cl_fwd,
        "channels-last InstanceNorm2d forward (y, mean, rstd)",
        py::arg("x"), py::arg("eps"), py::arg("deterministic") = false);
  m.def("instnorm_cl_bwd", &instnorm_cl_bwd,
        "channels-last InstanceNorm2d backward", py::arg("x"), py::arg("dy"),
        py::arg("mean"), py::arg("rstd"), py::arg("deterministic") = false);
  m.def("zero_inject_fwd", &zero_inject_fwd, "sparse injection scatter");
  m.def("zero_inject_bwd", &zero_inject_bwd, "backward gather of inject");
  m.def("forward_splat", &forward_splat,
        "nearest-neighbour forward splat of a flow field (warm start); "
        "splits: 0 = planned source chunks, n = forced",
        py::arg("flow"), py::arg("splits") = 0);
  m.def("forward_splat_plan", &forward_splat_plan,
        "source chunk count G the splat uses for an (H, W) field",
        py::arg("H"), py::arg("W"), py::arg("splits") = 0);
  m.def("fb_consistency", &fb_consistency,
        "forward-backward consistency check of a bidirectional flow pair -> "
        "[occ_fw, occ_bw, res_fw, res_bw, stats]",
        py::arg("flow_fw"), py::arg("flow_bw"), py::arg("alpha1") = 0.01,
        py::arg("alpha2") = 0.5);
  m.def("gru_gate1_fwd", &gru_gate1_fwd, "fused GRU z/r gates + r*h");
  m.def("gru_gate1_bwd", &gru_gate1_bwd, "backward of gru_gate1");
  m.def("gru_gate2_fwd", &gru_gate2_fwd, "fused GRU tanh + lerp update");
  m.def("gru_gate2_bwd", &gru_gate2_bwd, "backward of gru_gate2");
  m.def("seq_loss_fwd", &seq_loss_fwd,
        "fused sequence loss forward -> [loss, epe, 1px, 3px, 5px]");
  m.def("seq_loss_bwd", &seq_loss_bwd,
        "fused sequence loss backward -> per-prediction grads");
  m.def("nconv_bwd_prep", &nconv_bwd_prep,
        "fused elementwise preamble of nconv backward (dnomin, ddenom)");
  m.def("nconv_bwd", &nconv_bwd,
        "fused normalized convolution backward (ddata, dconf, dweight)");
  m.def("nconv_supported", &nconv_supported,
        "is (Ci, Co, K) an entry of the normalized-convolution kernel table",
        py::arg("Ci"), py::arg("Co"), py::arg("K"));
  m.def("nconv_bwd_fused", &nconv_bwd_fused,
        "whole nconv layer backward -> (ddata, dconf, dweight, dbias); "
        "algo 0 = split kernels, 1 = fused kernel, -1 = automatic",
        py::arg("gout"), py::arg("gcout"), py::arg("out"), py::arg("cout"),
        py::arg("data"), py::arg("conf"), py::arg("weight"), py::arg("bias"),
        py::arg("eps"), py::arg("algo") = -1, py::arg("strip") = 0);
}
