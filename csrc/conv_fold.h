// Host side of the tap-folded small-Cin convolution path (forward variant of
// conv_gemm_fwd_kernel, conv_wrw_fold_kernel and its reduce, all in
// conv_gemm.hip): the envelope, the weight-gradient plan and the index maps
// of the folded weight pack and partials buffer. Plain C++ above the
// launchers, like conv_gemm.h, so tests/host/conv_fold_plan_check.cpp
// enumerates every index the kernels form without a GPU.
//
// A conv whose input has exactly 8 channels as the kernels see it (the
// callers zero-pad 2 or 3 real channels to 8) has one pixel per 16-byte
// staging piece. The generic kernels spend a whole 64-wide k-step on the 8
// channels of ONE tap; the folded path puts the KW taps of one kernel row
// into the eight pieces of a k-row instead:
//   k column = kx * 8 + c   (kx < KW <= 8, c < 8), one k-step per ky.
// A 7x7 conv walks 7 k-steps instead of 49, and the weight gradient stages
// dy 7 times (ky in the grid) or once (ky looped in the workgroup) instead
// of 49 times.
//
//   folded pack:     wpk[ky][o][kx*8 + c]              (KH, O, 64) bf16
//   folded partials: p[chunk][ky][orow][kx*8 + c]      (nchunk, KH,
//                    tiles_o*64, 64) fp32, then the bias partials tail
//                    (nchunk, tiles_o*64), as in ConvGeom::buffer_numel
#pragma once

#include "conv_gemm.h"

// ky accumulator sets the in-workgroup form keeps in registers
// (CF_MAXKY * 16 fp32 per lane)
#define CF_MAXKY 7

// single source, 8 channels in whole 16-byte pixels, KW taps fit the eight
// pieces of a k-row, same padding, stride 1 or 2 over the m grid of a
// direct conv (smode 0 / 1 of conv_gemm.hip)
inline bool flowhip_conv_fold_envelope(const ConvGeom& g) {
  if (g.two_source() || g.Cin != 8) return false;
  if (g.ld_x < 8 || g.ld_x % 8 != 0) return false;
  if (g.KH < 1 || g.KW < 1 || g.KW > 8) return false;
  if (g.padH != g.KH / 2 || g.padW != g.KW / 2) return false;
  if (g.sH < 1 || g.sH > 2 || g.sW < 1 || g.sW > 2) return false;
  if (g.Mtot < 1 || g.Cout < 1) return false;
  if (g.sH == 1 && g.sW == 1) return g.HH == g.srcH && g.WW == g.srcW;
  return g.HH == (g.srcH + 2 * g.padH - g.KH) / g.sH + 1 &&
         g.WW == (g.srcW + 2 * g.padW - g.KW) / g.sW + 1;
}

// the weight gradient stages dy in whole 16-byte pieces on top
inline bool flowhip_conv_fold_wrw_envelope(const ConvGeom& g) {
  return flowhip_conv_fold_envelope(g) && g.Cout % 8 == 0;
}

// ---- index maps (kernels and host check share them) ----------------------
__host__ __device__ inline long cf_pack_index(int ky, int o, int kx, int c,
                                              int O) {
  return ((long)ky * O + o) * 64 + kx * 8 + c;
}
// dw (Cout, Cin, KH, KW)
__host__ __device__ inline long cf_dw_index(int o, int c, int ky, int kx,
                                            int Cin, int KH, int KW) {
  return (((long)o * Cin + c) * KH + ky) * KW + kx;
}
__host__ __device__ inline long cf_partial_index(int chunk, int ky, int orow,
                                                 int col, int KH, int orows) {
  return ((((long)chunk * KH + ky) * orows) + orow) * 64 + col;
}
// offset inside the bias tail
__host__ __device__ inline long cf_bias_index(int chunk, int orow,
                                              int orows) {
  return (long)chunk * orows + orow;
}
// The accumulator element (i, j, r) of lane `lane` of wave `wave` (2x2
// waves of 32x32, 2x2 MFMA 16x16 tiles each) -> (o row, k column) of the
// workgroup's 64x64 tile.
__host__ __device__ inline int cf_acc_orow(int wave, int lane, int i, int r) {
  return (wave >> 1) * 32 + i * 16 + (lane >> 4) * 4 + r;
}
__host__ __device__ inline int cf_acc_col(int wave, int lane, int j) {
  return (wave & 1) * 32 + j * 16 + (lane & 15);
}
// bias partial (i) of a lane < 16 of an even wave -> o row of the tile
__host__ __device__ inline int cf_bias_orow(int wave, int lane, int i) {
  return (wave >> 1) * 32 + i * 16 + lane;
}

inline long cf_wpartials_numel(const ConvGeom& g, int nchunk) {
  return (long)nchunk * g.KH * g.tiles_o() * 64 * 64;
}
inline long cf_buffer_numel(const ConvGeom& g, int nchunk, bool want_bias) {
  return cf_wpartials_numel(g, nchunk) +
         (want_bias ? (long)nchunk * g.tiles_o() * 64 : 0);
}

// The folded weight-gradient plan. One kernel, two forms:
//   form 0: ky in the grid, (tiles_o, KH, nchunk) workgroups. dy is staged
//           KH times.
//   form 1: ky looped in the workgroup, (tiles_o, 1, nchunk). dy is staged
//           once per m-tile against KH x tiles and KH accumulator sets
//           (KH <= CF_MAXKY); filling the chip takes KH times the chunks,
//           and every chunk costs KH * tiles_o * 16 KB of partials.
//   form_req: -1 the rule, 0 | 1 forced. nchunk_req: 0 = the form's own
//   choice, else forced (clamped to [1, min(m-tiles, 4096)]).
// Returns the form, or -1 when form 1 is forced with KH > CF_MAXKY.
//
// Rule: form 0 everywhere. Measured on MI355X (tools/bench_conv_fold.py,
// partials + reduce, median of alternating rounds, min-max within 1%;
// profiles/README.md round 9), us per call at the best chunk count of each
// form, against the generic per-tap path:
//                      generic   form 0 (nchunk)   form 1 (nchunk)
//   fnet stem b6         798       171 (96)          315 (256)
//   cnet stem b3         405       108 (74)          219 (224)
//   convf1 3x56x128       59        29 (19)           61 (56)
// Form 1 stages 40% fewer bytes per m-tile but holds 112 accumulator
// registers (174 VGPRs, two waves per SIMD at most), and the chunk count
// that gives every CU a workgroup costs it 29 MB of partials on the stems;
// it never caught up, so it runs on request only (ky_form = 1).
// Form 0 chunk count: about two workgroups per CU (512, the generic path's
// target: fnet 259 us at 37 chunks, 174 at 74, 171 at 96, 225 at 160);
// past one workgroup per CU (256) only while a workgroup still walks 16
// m-tiles (convf1, 336 m-tiles: 29 us at 19 chunks, 30 at 21, 31 at 28, 35
// at 37, 42 at 56: every chunk is partials traffic). Never fewer than fill
// the chip once: a single chunk also sums all of M in one fp32 chain, which
// measured 3-5x the generic path's error on the small test shapes.
// Form 1 on request: one workgroup per CU (256 / tiles_o).
inline int flowhip_conv_fold_wrw_plan(const ConvGeom& g, int form_req,
                                      int nchunk_req, int* nchunk_out) {
  const long mtiles = (g.Mtot + 63) / 64;
  const int to = g.tiles_o();
  if (form_req == 1 && g.KH > CF_MAXKY) return -1;
  const int form = form_req == 1 ? 1 : 0;
  long n = nchunk_req;
  if (nchunk_req <= 0) {
    if (form == 1) {
      n = cg_cdiv(256, to);
    } else {
      n = cg_cdiv(512, to * g.KH);
      const long once = cg_cdiv(256, to * g.KH);
      if (n > mtiles / 16) n = mtiles / 16 > once ? mtiles / 16 : once;
    }
  }
  if (n > 4096) n = 4096;
  if (n > mtiles) n = mtiles;
  if (n < 1) n = 1;
  *nchunk_out = (int)n;
  return form;
}

// workgroups of the planned grid along y (x = tiles_o, z = nchunk), and the
// [ky0, ky0 + nky) range workgroup row `by` owns
inline int cf_grid_y(const ConvGeom& g, int form) {
  return form == 1 ? 1 : g.KH;
}
__host__ __device__ inline int cf_ky0(int form, int by) {
  return form == 1 ? 0 : by;
}
__host__ __device__ inline int cf_nky(int form, int KH) {
  return form == 1 ? KH : 1;
}

// Calls that share a weight (convf1 over the refinement iterations) sum
// their partials in one buffer, reduced once. Measured for convf1, 12 calls
// per backward pass at 3x56x128 (tools/bench_conv_fold.py --accumulate,
// profiles/README.md round 9), in us per pass: form 0 accumulating 222,
// form 0 one-shot partials each with a finish into the running dW 357;
// the generic path's accumulating pass is 623.
inline bool flowhip_conv_fold_accumulate_wins() { return true; }

#if defined(__HIPCC__) || defined(__HIP_PLATFORM_AMD__)
// conv_gemm.hip. form / nchunk: as planned by flowhip_conv_fold_wrw_plan.
void flowhip_conv_fold_wrw_partials_launch(const void* dy, const void* x,
                                           float* partials, bool want_bias,
                                           const void* zpage,
                                           const ConvGeom& g, int nchunk,
                                           int form, bool accumulate,
                                           hipStream_t stream);
// reads Cin, Cout, KH, KW of g only
void flowhip_conv_fold_wrw_finish_launch(const float* partials, float* dw,
                                         float* dbias, const ConvGeom& g,
                                         int nchunk, bool accumulate,
                                         hipStream_t stream);
#endif
