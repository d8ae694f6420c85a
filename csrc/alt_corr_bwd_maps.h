// Index maps of the on-demand correlation lookup's backward
// (alt_corr_bwd.hip), as plain host/device functions so a host program
// (tests/host/alt_corr_bwd_maps_check.cpp) can enumerate every address the
// kernels will form before they run on a GPU.
//
// Forward geometry (alt_corr.hip), per (target pixel, level l): the level
// coordinate c = coord / 2^l is clamped IN FLOAT to [-(R+2), extent+R+1],
// the (K+1) x (K+1) patch (K = 2R+1) starts at origin o = floor(c) - R and
// output tap (a, c) blends patch positions (c..c+1, a..a+1) with weights
// (wy0, wy1) x (wx0, wx1), w1 = c - floor(c), w0 = 1 - w1. The backward is
// that blend transposed: patch position (j, a) collects the <= 4 taps
// (a - da, j - dj), da, dj in {0, 1}, that blended it.
//
// Tiled scatter: a workgroup owns ACB_TILE x ACB_TILE target pixels, one
// level and one 64-channel slice. It sums the tile's contributions per cell
// of a box of box x box level cells, box = K + 1 + ACB_BOX_EXTRA, anchored
// at max(0, min origin) over the tile's pixels whose window meets the map,
// and adds each touched cell to the global accumulator once. With smooth
// flow the 4 x 4 pixels' origins span <= 4 cells, so everything lands in
// the box; a cell outside it ("spill") goes straight to the global
// accumulator. Box row `by` belongs to wave by % ACB_WAVES (spilled map
// rows likewise, by the non-negative modulus of yy - ay), so one cell's sum
// is formed by one wave.
#pragma once

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#include <math.h>

#define ACB_TILE 4
#define ACB_NPIX (ACB_TILE * ACB_TILE)
#define ACB_BOX_EXTRA 4
#define ACB_MAX_BOX (2 * 4 + 2 + ACB_BOX_EXTRA)  // 14 at R = 4
#define ACB_SLICE 64                             // channels per workgroup
#define ACB_WAVES 4
#define ACB_MAX_K2 81
#define ACB_MAX_NPOS 100

// Clamped level coordinate -> patch origin and the two blend weights of one
// axis. fminf/fmaxf replace NaN by the bound, so `c` may be anything; the
// result is a finite origin in [-(2R+2), extent+1] (the int conversion never
// sees a value outside that band).
__host__ __device__ inline void acb_axis(float c, int extent, int R, int* o,
                                         float* w0, float* w1) {
  c = fminf(fmaxf(c, -(float)(R + 2)), (float)(extent + R + 1));
  const float f = floorf(c);
  *o = (int)f - R;
  *w1 = c - f;
  *w0 = 1.0f - *w1;
}

__host__ __device__ inline bool acb_in_map(int xx, int yy, int Wl, int Hl) {
  return (xx >= 0) & (xx < Wl) & (yy >= 0) & (yy < Hl);
}

// does the window [o, o+K] of one axis meet [0, extent)?
__host__ __device__ inline bool acb_axis_hits(int o, int K, int extent) {
  return (o + K >= 0) & (o < extent);
}

// Tap list of patch position (j = row, a = column), 0 <= j, a <= K. Slot
// s = dj * 2 + da (dj: uses wy1, da: uses wx1) is output tap
// (a - da, j - dj); tap[s] = its index into the level's K*K cotangent block
// (x-offset-major: a_out * K + c_out), 0 where the slot does not exist.
// Returns the mask of existing slots (1, 2 or 4 bits set). Fixed slots keep
// every array index a compile-time constant in the kernels (no scratch).
__host__ __device__ inline int acb_taps(int j, int a, int K, int tap[4]) {
  int mask = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int c = j - (s >> 1), ao = a - (s & 1);
    const bool ok = (c >= 0) & (c < K) & (ao >= 0) & (ao < K);
    tap[s] = ok ? ao * K + c : 0;
    mask |= ok ? 1 << s : 0;
  }
  return mask;
}

// element offset of tap `ch` (0 <= ch < C = L*K2) of pixel i, batch b, in
// the cotangent: NCHW (B, C, P) or NHWC rows of stride ldc >= C (the pad
// tail [C, ldc) is never addressed).
__host__ __device__ inline long acb_grad_off(int b, int i, int ch, int P,
                                             int C, int cl, int ldc) {
  return cl ? ((long)b * P + i) * ldc + ch : ((long)b * C + ch) * P + i;
}

// tile index -> (batch, first pixel row, first pixel column)
__host__ __device__ inline void acb_tile_decode(int tile, int H, int W,
                                                int* b, int* ty, int* tx) {
  const int tw = (W + ACB_TILE - 1) / ACB_TILE;
  const int th = (H + ACB_TILE - 1) / ACB_TILE;
  *b = tile / (tw * th);
  const int r = tile - *b * (tw * th);
  *ty = (r / tw) * ACB_TILE;
  *tx = (r - (r / tw) * tw) * ACB_TILE;
}

__host__ __device__ inline int acb_box_side(int R) {
  return 2 * R + 2 + ACB_BOX_EXTRA;
}

// Box anchor of one axis: fold one pixel's origin into the running minimum
// (start from ACB_NO_ANCHOR); only windows that meet the map take part.
#define ACB_NO_ANCHOR 0x3fffffff
__host__ __device__ inline int acb_anchor_fold(int cur, int o) {
  const int v = o < 0 ? 0 : o;
  return v < cur ? v : cur;
}

// in-map cell (xx, yy) -> slot by*box + bx of the box anchored at (ax, ay),
// or -1 when the cell lies outside the box (spill).
__host__ __device__ inline int acb_box_slot(int xx, int yy, int ax, int ay,
                                            int box) {
  const int bx = xx - ax, by = yy - ay;
  if ((bx < 0) | (bx >= box) | (by < 0) | (by >= box)) return -1;
  return by * box + bx;
}

// Can the in-map part of the window [o, o+K] of one axis leave a box of side
// `box` anchored at `anchor`? The anchor is the minimum clamped origin, so
// only the far edge can. A pixel for which neither axis spills is skipped
// by the spill pass as a whole.
__host__ __device__ inline bool acb_axis_spills(int o, int K, int extent,
                                                int anchor, int box) {
  const int e = o + K < extent - 1 ? o + K : extent - 1;
  return e >= anchor + box;
}

// wave that owns map row yy of a box anchored at row ay (non-negative
// modulus: spilled rows above the box have yy < ay)
__host__ __device__ inline int acb_row_owner(int yy, int ay) {
  int m = (yy - ay) % ACB_WAVES;
  return m < 0 ? m + ACB_WAVES : m;
}

// finalize: does level l (extent Hl x Wl) hold a cell for level-0 (y, x)?
// Floor-mode pooling drops the odd last row/column, so (y >> l) can fall
// off the level.
__host__ __device__ inline bool acb_fin_member(int y, int x, int l, int Hl,
                                               int Wl) {
  return ((y >> l) < Hl) & ((x >> l) < Wl);
}
