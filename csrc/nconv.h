// Host side of the normalized-convolution family (nconv.hip,
// nconv_bwd_fused.hip): the one description of a layer's geometry, the one
// table of (K, Ci, Co) the kernels are instantiated for, the launch plans,
// and the launcher prototypes. Included by the two .hip files and by
// bindings.cpp, so the compiler checks every call. Everything above the
// launchers is plain C++ that a host program compiles without HIP
// (tests/host/nconv_plan_check.cpp).
#pragma once

// data / conf are (N, Ci, H, W), weight is (Co, Ci, K, K); stride 1, zero
// padding K/2, fp32.
struct NConvGeom {
  int N, Ci, Co, H, W, K;
};

// The envelope: every dispatcher expands this list and nothing else.
// fwd<K,CI,CO> and fused<K,CI,CO> are instantiated per entry; bwd_data<K,CO>
// and wrw<K,CI> are its projections.
#define FLOWHIP_NCONV_TABLE(X)                                              \
  X(5, 1, 1) X(5, 1, 2) X(5, 1, 4) X(5, 2, 1) X(5, 2, 2) X(5, 2, 4)         \
  X(5, 4, 2) X(5, 4, 4)                                                     \
  X(3, 1, 1) X(3, 1, 2) X(3, 1, 4) X(3, 2, 1) X(3, 2, 2) X(3, 2, 4)         \
  X(3, 4, 2) X(3, 4, 4) X(3, 8, 2)                                          \
  X(1, 1, 1) X(1, 1, 2) X(1, 2, 1) X(1, 2, 2) X(1, 4, 2)

inline bool flowhip_nconv_supported(int Ci, int Co, int K) {
#define FLOWHIP_NCONV_CASE_IN(KK, CIV, COV) \
  if (K == KK && Ci == CIV && Co == COV) return true;
  FLOWHIP_NCONV_TABLE(FLOWHIP_NCONV_CASE_IN)
#undef FLOWHIP_NCONV_CASE_IN
  return false;
}

// What every launcher accepts: a table entry and whole float4 rows (each
// thread owns 4 adjacent pixels; a chunk is all inside the image or all
// outside). Anything else returns false and launches nothing.
inline bool flowhip_nconv_launchable(const NConvGeom& g) {
  return g.W % 4 == 0 && flowhip_nconv_supported(g.Ci, g.Co, g.K);
}

// Output tile of one 256-thread workgroup: 16 lanes x 4 px cover a row.
constexpr int NCONV_TW = 64;
constexpr int NCONV_TH = 16;

constexpr int nconv_cdiv(int a, int b) { return (a + b - 1) / b; }

// wrw tile height by channel count: as tall as the LDS budget allows —
// the per-co wave-shuffle reduction (6 shfl per accumulator) amortizes
// over TH*TW pixels, so taller tiles cut its share 2-4x.
constexpr int flowhip_nconv_wrw_th(int Ci) {
  return Ci == 1 ? 64 : Ci == 2 ? 48 : Ci == 4 ? 32 : 16;
}

// Workgroups (= partials rows of Co*Ci*K*K) of the weight-gradient launch.
inline int flowhip_nconv_wrw_nblocks(const NConvGeom& g) {
  return nconv_cdiv(g.W, NCONV_TW) *
         nconv_cdiv(g.H, flowhip_nconv_wrw_th(g.Ci)) * g.N;
}

// Number of workgroups (= partials rows) of the fused launch, 0 outside
// the envelope. strip <= 0 picks the strip length: about 384 workgroups
// (1.5 per CU) when the image has that many tiles. Shorter strips pay the
// per-workgroup reduction more often, longer ones leave CUs idle
// (bench_nconv_bwd.py --strips: 4 / 7 / 14 tile rows at the flagship).
inline int flowhip_nconv_bwd_fused_plan(const NConvGeom& g, int* strip) {
  if (!flowhip_nconv_launchable(g)) return 0;
  const int ntx = nconv_cdiv(g.W, NCONV_TW), nty = nconv_cdiv(g.H, NCONV_TH);
  int st = *strip;
  if (st <= 0) {
    st = (ntx * nty * g.N) / 384;
    if (st < 1) st = 1;
    if (st > 8) st = 8;
  }
  if (st > nty) st = nty;
  *strip = st;
  return ntx * nconv_cdiv(nty, st) * g.N;
}

// Columns of a fused partials row: [Co*Ci*K*K dweight sums | Co sums of
// cout*gcout | Co sums of gout].
inline int flowhip_nconv_bwd_fused_ncol(const NConvGeom& g) {
  return g.Co * g.Ci * g.K * g.K + 2 * g.Co;
}

// Launchers, defined in the .hip files. Fenced like those of conv_gemm.h:
// a plain host compiler sees the geometry, the table and the plans only.
// Each that takes a geometry returns false, having launched nothing,
// outside flowhip_nconv_launchable.
#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
#include <hip/hip_runtime.h>

// nconv.hip. bias: (Co) or nullptr.
bool flowhip_nconv_fwd_launch(const float* data, const float* conf,
                              const float* weight, const float* bias,
                              float* out, float* cout, const NConvGeom& g,
                              hipStream_t stream);
bool flowhip_nconv_bwd_data_launch(const float* dnomin, const float* ddenom,
                                   const float* data, const float* conf,
                                   const float* weight, float* ddata,
                                   float* dconf, const NConvGeom& g,
                                   hipStream_t stream);
// partials: flowhip_nconv_wrw_nblocks(g) rows of Co*Ci*K*K
bool flowhip_nconv_wrw_launch(const float* dnomin, const float* ddenom,
                              const float* data, const float* conf,
                              float* partials, float* dweight,
                              const NConvGeom& g, hipStream_t stream);
// elementwise over `total` values of (N, Co, H, W) planes, so it has no
// geometry to refuse; gcout, bias may be nullptr
void flowhip_nconv_bwd_prep_launch(const float* gout, const float* gcout,
                                   const float* out, const float* cout,
                                   const float* wsum, const float* bias,
                                   float* dnomin, float* ddenom, long total,
                                   long plane, int Co, float eps,
                                   hipStream_t stream);
// nconv_bwd_fused.hip. partials: flowhip_nconv_bwd_fused_plan(g, &strip)
// rows of flowhip_nconv_bwd_fused_ncol(g); gout, gcout, bias, dbias may be
// nullptr.
bool flowhip_nconv_bwd_fused_launch(
    const float* gout, const float* gcout, const float* out,
    const float* cout, const float* data, const float* conf,
    const float* weight, const float* bias, float* ddata, float* dconf,
    float* partials, float* dweight, float* dbias, const NConvGeom& g,
    int strip, float eps, hipStream_t stream);
#endif
