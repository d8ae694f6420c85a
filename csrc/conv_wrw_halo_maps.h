// Address maps of the halo-staged weight-gradient kernel
// (conv_wrw_halo.hip), as plain host/device functions so a host program
// (tests/host/wrw_halo_maps_check.cpp) can enumerate every address the
// kernel will form before it runs on a GPU. The tile geometry's other
// host-side consumer, the split-M chunk policy (wh_nchunk), sits at the
// end.
//
// One workgroup (256 threads, 4 waves) walks pixel tiles of WH_TH x WH_TW
// output pixels of one image. Per pixel tile it stages two LDS images of
// 128-byte pixel rows (64 bf16 channels each):
//   dy image : WH_TH x WH_TW pixels            (pix = ty*WH_TW + tx)
//   x  image : (WH_TH+KH-1) x LW px            (pix = py*LW + px), halo;
//              LW = WH_TW+KW-1 rounded up to a multiple of 8 (40 for KW 3
//              and 5, 32 for KW 1): a 64-piece wave instruction never
//              crosses an image row, and a row offset (ks+ky)*LW does not
//              reach the swizzle bits, so one address per kx serves every
//              k-step and every ky. Columns past WH_TW+KW-1 hold zeros and
//              are never read.
// A row is cut into four 32-byte chunks (16 channels). Chunk cb of pixel
// pix is stored at chunk position cb ^ wh_swz(pix): a transposed read of
// one 32-lane half touches 8 CONSECUTIVE pixels x 32 B, and
// (pix&1)*4 + (cb ^ ((pix>>1)&3)) is a bijection of any 8 consecutive
// pixels onto the eight 32-byte windows of the 256-byte bank row, so the
// reads are conflict-free for every tap shift (a tap only adds a constant
// to pix). The swizzle is applied to the SOURCE address of the
// global_load_lds piece; the LDS destination stays lane-linear.
//
// Staging piece p (16 B): pix = p >> 3, slot = p & 7, LDS byte p * 16,
// channels ((slot>>1) ^ wh_swz(pix))*16 + (slot&1)*8 .. +8 of the slab.
//
// k-step ks (0..WH_TH-1) contracts the 32 pixels of tile row ks. MFMA k
// slot s = g*8 + h*4 + q (g = lane>>4, h = which of the two transposed
// reads, q = row inside the 4x16 block) holds tile column
// tx = h*16 + g*4 + q, so the two lane groups of a 32-lane half read 8
// consecutive pixels. dy and x use the same slot->pixel map; a tap
// (ky, kx) reads x pixel (ks+ky)*LW + tx + kx.
#pragma once

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#define WH_TH 4
#define WH_TW 32
#define WH_THREADS 256
#define WH_DY_PIECES (WH_TH * WH_TW * 8)
#define WH_DY_BYTES (WH_DY_PIECES * 16)

__host__ __device__ inline int wh_lw(int KW) {
  return (WH_TW + KW - 1 + 7) / 8 * 8;
}
__host__ __device__ inline int wh_lh(int KH) { return WH_TH + KH - 1; }
// x image pieces: a multiple of 64 (whole wave instructions) as LW % 8 == 0
__host__ __device__ inline int wh_x_pieces(int KH, int KW) {
  return wh_lh(KH) * wh_lw(KW) * 8;
}
__host__ __device__ inline int wh_lds_bytes(int KH, int KW) {
  return WH_DY_BYTES + wh_x_pieces(KH, KW) * 16;
}

__host__ __device__ inline unsigned wh_swz(unsigned pix) {
  return (pix >> 1) & 3u;
}
// channel offset (inside the 64-channel slab) a staging piece carries
__host__ __device__ inline int wh_piece_chan(int piece) {
  const unsigned pix = (unsigned)piece >> 3, slot = (unsigned)piece & 7u;
  return (int)((((slot >> 1) ^ wh_swz(pix)) << 4) + ((slot & 1u) << 3));
}

// dy staging source: element offset into dy (N*H*W, Cout), or -1 for the
// zero page. (n, y0, x0) = pixel-tile origin, o0 = first output channel.
__host__ __device__ inline long wh_dy_src(int piece, int n, int y0, int x0,
                                          int H, int W, int Cout, int o0) {
  const int pix = piece >> 3;
  const int gy = y0 + pix / WH_TW, gx = x0 + pix % WH_TW;
  const int o = o0 + wh_piece_chan(piece);
  if (gy >= H || gx >= W || o >= Cout) return -1;
  return (((long)n * H + gy) * W + gx) * Cout + o;
}

// x staging source: which = 0 zero page, 1 x (row stride ld_x), 2 x2.
// Returns the element offset into that tensor.
__host__ __device__ inline long wh_x_src(int piece, int n, int y0, int x0,
                                         int H, int W, int KH, int KW,
                                         int ld_x, int ld_x2, int C1,
                                         int Cin, bool has_x2, int c0,
                                         int* which) {
  const int LW = wh_lw(KW);
  const int pix = piece >> 3;
  const int py = pix / LW, px = pix - py * LW;
  const int gy = y0 + py - KH / 2, gx = x0 + px - KW / 2;
  const int c = c0 + wh_piece_chan(piece);
  *which = 0;
  if (px >= WH_TW + KW - 1 || gy < 0 || gy >= H || gx < 0 || gx >= W ||
      c >= Cin)
    return 0;
  const long p = ((long)n * H + gy) * W + gx;
  if (!has_x2 || c < C1) {
    *which = 1;
    return p * ld_x + c;
  }
  *which = 2;
  return p * ld_x2 + (c - C1);
}

// The same staging maps in the per-thread form the kernel runs. Thread tid
// stages pieces tid + 256*j: pix = (tid>>3) + 32*j, so its channel offset
// is the same for every j, a dy piece j is tile row j at column tid>>3,
// and the x halo pixel advances by 32 with at most one row wrap
// (32 <= LW <= 40). With C1 % 64 == 0 a 64-channel slab comes wholly from
// x or wholly from x2, so the source tensor is chosen per workgroup.
struct WhStage {
  int tx;    // dy tile column
  int chan;  // channel offset of this thread's pieces inside the slab
  int px0, py0;  // halo pixel of x piece j = 0
};
__host__ __device__ inline WhStage wh_stage_init(int tid, int KW) {
  WhStage S;
  S.tx = tid >> 3;
  S.chan = wh_piece_chan(tid);
  S.py0 = (tid >> 3) / wh_lw(KW);
  S.px0 = (tid >> 3) - S.py0 * wh_lw(KW);
  return S;
}
__host__ __device__ inline long wh_dy_src_thr(const WhStage& S, int j, int n,
                                              int y0, int x0, int H, int W,
                                              int Cout, int o0) {
  const int gy = y0 + j, gx = x0 + S.tx, o = o0 + S.chan;
  if (gy >= H || gx >= W || o >= Cout) return -1;
  return (long)(((n * H + gy) * W) + gx) * Cout + o;
}
__host__ __device__ inline void wh_x_step(int& px, int& py, int KW) {
  px += 32;
  if (px >= wh_lw(KW)) {
    px -= wh_lw(KW);
    ++py;
  }
}
// element offset into the slab's source tensor (row stride ld, first slab
// channel at tensor channel cbase), or -1 for the zero page
__host__ __device__ inline long wh_x_src_thr(const WhStage& S, int px, int py,
                                             int n, int y0, int x0, int H,
                                             int W, int KH, int KW, int ld,
                                             int cbase, int c0, int Cin) {
  const int gy = y0 + py - KH / 2, gx = x0 + px - KW / 2;
  if (px >= WH_TW + KW - 1 || gy < 0 || gy >= H || gx < 0 || gx >= W ||
      c0 + S.chan >= Cin)
    return -1;
  return (long)(((n * H + gy) * W) + gx) * ld + (cbase + S.chan);
}

// tile column a lane addresses in transposed read h (0|1) of a k-step
__host__ __device__ inline int wh_tr_tx(int lane, int h) {
  return h * 16 + (lane >> 4) * 4 + ((lane >> 2) & 3);
}
// byte address inside an image of the 8 bytes lane `lane` supplies to a
// transposed read of channel block cb (16 channels) at image pixel pix
__host__ __device__ inline unsigned wh_tr_addr(unsigned pix, int cb,
                                               int lane) {
  return pix * 128u + (((unsigned)cb ^ wh_swz(pix)) << 5) +
         ((unsigned)lane & 3u) * 8u;
}
__host__ __device__ inline unsigned wh_dy_pix(int ks, int tx) {
  return (unsigned)(ks * WH_TW + tx);
}
__host__ __device__ inline unsigned wh_x_pix(int ks, int tx, int ky, int kx,
                                             int KW) {
  return (unsigned)((ks + ky) * wh_lw(KW) + tx + kx);
}

// The same addresses in the form the kernel runs: everything that depends
// on the lane is computed once (4 + KW registers); the k-step adds a
// wave-uniform row offset; h and ky are compile-time constants that land
// in the ds_read immediate offset. With tx = wh_tr_tx(lane, 0) (h adds 16
// and a row adds a multiple of 8 pixels, neither reaches the swizzle):
//   swz(row + kx + tx) = ((kx>>1) + ((tx + (kx&1)) >> 1)) & 3
struct WhLane {
  unsigned dy[4];  // per o block i: tx*128 + p8 + swizzled chunk
  unsigned x[5];   // per kx, for the lane's c block, incl. the kx pixels
};
__host__ __device__ inline WhLane wh_lane_init(int lane, int cbx) {
  WhLane L;
  const unsigned tx = (unsigned)wh_tr_tx(lane, 0);
  const unsigned base = tx * 128u + ((unsigned)lane & 3u) * 8u;
  for (int i = 0; i < 4; ++i)
    L.dy[i] = base + (((unsigned)i ^ ((tx >> 1) & 3u)) << 5);
  for (unsigned kx = 0; kx < 5; ++kx)
    L.x[kx] = base + kx * 128u +
              (((unsigned)cbx ^ (((kx >> 1) + ((tx + (kx & 1u)) >> 1)) & 3u))
               << 5);
  return L;
}
// compile-time parts (ds_read immediate offsets) and per-k-step row offsets
__host__ __device__ constexpr unsigned wh_dy_imm(int h) {
  return (unsigned)h * 16u * 128u;
}
__host__ __device__ constexpr unsigned wh_x_imm(int h, int ky, int KW) {
  return (unsigned)(ky * ((WH_TW + KW - 1 + 7) / 8 * 8) + h * 16) * 128u;
}
__host__ __device__ constexpr unsigned wh_dy_kstep(int ks) {
  return (unsigned)ks * WH_TW * 128u;
}
__host__ __device__ constexpr unsigned wh_x_kstep(int ks, int KW) {
  return (unsigned)ks * ((WH_TW + KW - 1 + 7) / 8 * 8) * 128u;
}
__host__ __device__ inline unsigned wh_dy_addr(const WhLane& L, int ks, int h,
                                               int i) {
  return L.dy[i] + wh_dy_kstep(ks) + wh_dy_imm(h);
}
__host__ __device__ inline unsigned wh_x_addr(const WhLane& L, int ks, int h,
                                              int ky, int kx, int KW) {
  return L.x[kx] + wh_x_kstep(ks, KW) + wh_x_imm(h, ky, KW);
}

// split-M chunk count of the halo path. Model, per call:
//   operands  = M * tiles * (64 + 64*halo) * 2 B   (halo = LH*LW/(TH*TW):
//               1.59 for 3x3, 1.13 for 1x5, 2.0 for 5x1), independent of
//               nchunk;
//   partials  = nchunk * tiles * 64*64 * KYX * 8 B (written, then read by
//               the reduce).
// Measured (tools/bench_wrw.py, chunk sweep at the flagship inventory): the
// time per call is flat-bottomed around tiles * nchunk ~ 192 workgroups
// for every routed class (12 x 16, 8 x 24, 24 x 8 in the update block,
// 4 x 48..64 in the 96-channel encoder stage). Fewer workgroups leave CUs
// idle (each workgroup has its CU to itself: 92-96 KB of LDS); more pay
// for partials faster than they shorten the per-workgroup tile walk —
// twice the chunks measured 1.2-1.5x slower.
__host__ __device__ inline int wh_nchunk(long ptiles, int tiles) {
  long n = (192 + tiles / 2) / tiles;
  if (n > ptiles) n = ptiles;
  if (n < 1) n = 1;
  return (int)n;
}
