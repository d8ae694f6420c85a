// Host side of the implicit-GEMM convolution family (conv_gemm.hip,
// conv_halo.hip, conv_wrw_halo.hip): the one description of a conv's
// geometry, the weight-gradient plan, and the launcher prototypes.
// Included by the three .hip files and by bindings.cpp, so the compiler
// checks every call. Everything above the launchers is plain C++ that a
// host program compiles without HIP (tests/host/conv_plan_check.cpp).
#pragma once

#include "conv_wrw_halo_maps.h"  // WH_TH, WH_TW, wh_nchunk

inline int cg_cdiv(int a, int b) { return (a + b - 1) / b; }

// channel padding of the packed weights and of the weight partials
inline int cg_cpad(int Cin) { return cg_cdiv(Cin, 64) * 64; }

// A conv as the kernels see it. The m axis walks Mtot = N * HH * WW pixels:
// the output of a direct conv and of the weight gradient, the input
// gradient of the strided-transposed form. (srcH, srcW) are the dims of the
// tensor the taps read. Channels [0, C1) come from x (row stride ld_x),
// [C1, Cin) from x2 (row stride ld_x2); C1 == Cin with a single source.
struct ConvGeom {
  long Mtot;
  int HH, WW, srcH, srcW, sH, sW, ld_x, ld_x2, C1, Cin, Cout, cpad, KH, KW,
      padH, padW;

  int N() const { return (int)(Mtot / ((long)HH * WW)); }
  int tiles_o() const { return cg_cdiv(Cout, 64); }
  int tiles_c() const { return cg_cdiv(cpad, 64); }
  bool two_source() const { return Cin > C1; }

  // Weight-gradient partials buffer: (nchunk, KH*KW, tiles_o*64, cpad)
  // weight partials, then (nchunk, tiles_o*64) bias partials at the tail.
  long wpartials_numel(int nchunk) const {
    return (long)nchunk * KH * KW * tiles_o() * 64 * cpad;
  }
  long buffer_numel(int nchunk, bool want_bias) const {
    return wpartials_numel(nchunk) +
           (want_bias ? (long)nchunk * tiles_o() * 64 : 0);
  }
  float* biasp(float* partials, int nchunk) const {
    return partials + wpartials_numel(nchunk);
  }
  const float* biasp(const float* partials, int nchunk) const {
    return partials + wpartials_numel(nchunk);
  }

  // The tap envelope of the halo-staged kernels (forward / backward-data
  // in conv_halo.hip, weight gradient in conv_wrw_halo.hip): stride 1,
  // same padding, 3x3 / 1x5 / 5x1, whole 64-channel slabs.
  bool halo_envelope() const {
    return sH == 1 && sW == 1 && srcH == HH && srcW == WW &&
           padH == KH / 2 && padW == KW / 2 &&
           ((KH == 3 && KW == 3) || (KH == 1 && KW == 5) ||
            (KH == 5 && KW == 1)) &&
           cpad % 64 == 0;
  }
  // What the weight-gradient halo kernel needs on top: whole 16-byte dy
  // pieces, one source tensor per 64-channel slab, and pixels its staging
  // maps can index in 32 bits.
  bool wrw_halo_envelope() const {
    return halo_envelope() && Cout % 8 == 0 &&
           (!two_source() || C1 % 64 == 0) && Mtot <= 0x7fffffffL;
  }
};

// Chooses the weight-gradient path and its split-M chunk count; the caller
// sizes the partials buffer (ConvGeom::buffer_numel) from the result.
//   algo: -1 auto, 0 generic per-tap kernel, 1 halo-staged kernel
//         (conv_wrw_halo.hip). Returns the path taken (0 | 1), or -1 when
//         algo == 1 was forced on a shape outside the halo envelope.
//   nchunk_req: 0 = the path's own choice, else forced (clamped).
inline int flowhip_conv_gemm_wrw_plan(const ConvGeom& g, int algo,
                                      int nchunk_req, int* nchunk_out) {
  const bool eligible = g.wrw_halo_envelope();
  if (algo == 1 && !eligible) return -1;
  const long ptiles = eligible ? (long)g.N() * cg_cdiv(g.HH, WH_TH) *
                                     cg_cdiv(g.WW, WH_TW)
                               : 0;
  // auto follows tools/bench_wrw.py (profiles/README.md round 3): the halo
  // kernel wins where one staged tile pair feeds enough output tiles or a
  // long pixel walk — 8+ output tiles (update block: 256->192, 256->126,
  // 128->256 3x3 and the 384-channel 1x5 / 5x1 GRU convs, 6-22% faster),
  // or 4+ output tiles over 672+ pixel tiles (96-channel encoder stage,
  // 20-39%). It measured SLOWER, and stays on the generic kernel, for
  // 128->64 and 256->2 at 56x128 (2-4 output tiles: too few workgroups
  // for a kernel that owns its CU) and for the 64- and 128-channel
  // encoder stages. The rule is fitted to those measured classes only: the
  // 672 threshold is the batch-3 96-channel encoder shape, the smallest
  // 4-tile class that won; nothing between the measured points is known.
  const int tiles = g.tiles_o() * g.tiles_c();
  const bool wins = tiles >= 8 || (tiles >= 4 && ptiles >= 672);
  const bool halo = eligible && (algo == 1 || (algo == -1 && wins));
  if (halo) {
    long n = nchunk_req > 0 ? nchunk_req : wh_nchunk(ptiles, tiles);
    if (n > ptiles) n = ptiles;
    if (n > 4096) n = 4096;
    *nchunk_out = (int)n;
    return 1;
  }
  // generic: split M only as much as needed to fill the chip (~2 blocks
  // per CU); more chunks = more fp32 partial traffic + a longer reduce
  const int base_tiles = tiles * g.KH * g.KW;
  int nchunk = nchunk_req > 0 ? nchunk_req
                              : (512 + base_tiles - 1) / base_tiles;
  if (nchunk < 1) nchunk = 1;
  if (nchunk > 64) nchunk = 64;  // encoder shapes: few tiles, huge M
  // never more chunks than 64-row m-tiles
  const long mtiles = (g.Mtot + 63) / 64;
  if (nchunk > mtiles) nchunk = (int)mtiles;
  *nchunk_out = nchunk;
  return 0;
}

// Whether calls that share a weight should sum their partials in one
// buffer (partials launch with accumulate, one finish at the end) or run
// one-shot partials and add each call's reduce to a running dW (finish
// with accumulate). Measured per backward pass of 12 calls at 3x56x128 on
// MI355X (tools/bench_wrw.py --accumulate, median of 5 alternating rounds,
// min-max within 1%; profiles/README.md round 5). Columns: 12 one-shot
// calls + 11 fp32 adds of dW and dbias | 12 accumulating calls + 1 finish
// | 12 one-shot partials each with a finish into the running dW; in us.
//   generic path: accumulating partials wins on every shape
//     128->64 3x3    428 | 215 | 385      256->2 3x3    453 | 321 | 414
//     324->256 1x1   491 | 320 | 456      8->128 7x7    702 | 614 | 666
//   halo path: accumulating partials loses on every shape, the finish
//   into the running dW wins
//     256->192 3x3   705 |  965 | 665     384->256 1x5  818 |  939 | 774
//     256->126 3x3   593 |  817 | 554     384->256 5x1  911 | 1037 | 867
//     128->256 3x3   595 |  741 | 554     384->128 1x5  567 |  643 | 528
//                                         384->128 5x1  613 |  700 | 575
// The halo kernel owns its CU at one wave per SIMD, so nothing hides the
// latency of its epilogue's 16 * KYX loads per thread, and in the training
// step its 15-27 MB buffers leave the cache between two iterations: +41 us
// per launch in the kernel trace, against 13 us of reduce and 9 us of adds
// saved. The rule follows the two measured classes.
inline bool flowhip_conv_gemm_wrw_accumulate_wins(int path) {
  return path == 0;
}

// Launchers, defined in the .hip files. Fenced like the __host__ /
// __device__ markers of conv_wrw_halo_maps.h: a plain host compiler sees
// the geometry and the plan only.
#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
#include <hip/hip_runtime.h>

// conv_gemm.hip. smode: 0 stride-1 same padding, 1 strided direct, 2
// strided transposed (see the file's header). out2 / osplit: split output.
// fold: wpk is a folded pack and g is inside flowhip_conv_fold_envelope
// (conv_fold.h), which the caller checked.
void flowhip_conv_gemm_fwd_launch(const void* x, const void* x2,
                                  const void* wpk, const float* bias,
                                  void* out, void* out2, const void* zpage,
                                  const ConvGeom& g, int osplit, int act,
                                  int smode, hipStream_t stream,
                                  bool fold = false);
// conv_halo.hip. Returns false (nothing launched) outside its envelope or
// below its fill rule: the generic kernel takes the call.
bool flowhip_conv_halo_fwd_launch(const void* x, const void* x2,
                                  const void* wpk, const float* bias,
                                  void* out, const void* zpage,
                                  const ConvGeom& g, int act,
                                  hipStream_t stream);
// The weight gradient runs in two steps that share one partials buffer
// (layout: ConvGeom::buffer_numel). algo / nchunk: as returned by
// flowhip_conv_gemm_wrw_plan.
bool flowhip_conv_gemm_wrw_partials_launch(const void* dy, const void* x,
                                           const void* x2, float* partials,
                                           bool want_bias, const void* zpage,
                                           const ConvGeom& g, int nchunk,
                                           int algo, bool accumulate,
                                           hipStream_t stream);
// conv_wrw_halo.hip: the halo-staged partials kernel alone
bool flowhip_conv_wrw_halo_launch(const void* dy, const void* x,
                                  const void* x2, float* partials,
                                  float* biasp, const void* zpage,
                                  const ConvGeom& g, int nchunk,
                                  bool accumulate, hipStream_t stream);
// reads Cin, Cout, cpad, KH, KW of g only
void flowhip_conv_gemm_wrw_finish_launch(const float* partials, float* dw,
                                         float* dbias, const ConvGeom& g,
                                         int nchunk, bool accumulate,
                                         hipStream_t stream);
void flowhip_conv_gemm_pack_launch(const float* w, void* wpk, long total,
                                   int O, int I, int KH, int KW, int cpad,
                                   int flip, hipStream_t stream);
#endif
