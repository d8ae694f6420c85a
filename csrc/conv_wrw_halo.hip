// Halo-staged weight gradient for the stride-1 same-padding 3x3 / 1x5 /
// 5x1 convolutions (the envelope of conv_halo.hip's forward kernel).
//
//   dW[o, ky, kx, c] = sum_{n,y,x} dy[n, y, x, o] * x[n, y+ky-KH/2, x+kx-KW/2, c]
//
// The generic conv_gemm_wrw_kernel runs one workgroup per (o tile, c tile,
// TAP, chunk) and restages a dy tile and a tap-shifted x tile per 64
// pixels: every dy element is fetched tiles_c*KYX times and every x element
// tiles_o*KYX times. Here a workgroup owns one 64(o) x 64(c) output tile
// for ALL taps. Per pixel tile (WH_TH x WH_TW output pixels of one image)
// it stages the dy tile and ONE x halo tile, once each, and derives every
// tap's B operand from the halo image by a constant pixel offset in the
// transposed LDS read (ds_read_b64_tr_b16), one accumulator set per tap.
// Operand traffic falls by about KYX/halo (9/1.59 for 3x3, 5/1.13 for
// 1x5, 5/2 for 5x1) and the per-pixel-tile barrier pair is amortized over
// 4 * KYX * 4 MFMAs per wave instead of 8.
//
// Layout, swizzle and slot->pixel maps: conv_wrw_halo_maps.h (checked on
// the host by tests/host/wrw_halo_maps_check.cpp).
//
// Waves: 4, each owns all 64 o x its own 16 c (wave w = c block w): the dy
// fragments (8 reads per k-step) are shared by all taps, each tap adds 2
// x reads for 4 MFMAs -> 26 transposed reads per 36 MFMAs (3x3), all
// issued one k-step ahead of their MFMAs.
// Accumulators: KYX * 4 f32x4 = 144 (3x3) / 80 (1x5, 5x1) registers.
// LDS, double-buffered over pixel tiles: 2 x (16 KB dy + 30 KB (3x3) /
// 20 KB (1x5) / 32 KB (5x1) x) = 92 / 72 / 96 KB of the CU's 160 KB. The
// update-block shapes have only 168 pixel tiles, so the grid is about one
// workgroup per CU anyway (more chunks cost more in fp32 partials than
// they win); the next tile's staging overlaps this tile's MFMAs inside
// the workgroup instead of across workgroups.
//
// Contracts kept from the generic path: deterministic split-M fp32
// partials in the layout (CHUNKS, KYX, tiles_o*64, cpad) consumed by
// conv_gemm_wrw_reduce_kernel (no float atomics); the tc == 0 workgroups
// accumulate the bias gradient from the dy fragments they already hold.

#include "common.h"
#include "conv_gemm.h"

typedef __attribute__((ext_vector_type(4))) short wh_s16x4;
typedef __attribute__((ext_vector_type(8))) short wh_s16x8;

// Transposed LDS read issued from inline asm, waited for by WH_LGKM_WAIT.
// The compiler-tracked builtin form costs the double buffering: hipcc
// cannot tell which image an LDS read touches, so it drains vmcnt (the
// NEXT tile's global_load_lds pieces) before the first read of every tile.
// Only lgkmcnt(0) waits are used, so a scalar load the compiler may have
// in flight cannot make a counted wait return early.
// HAZARD: between WH_TR and landed() the destination register is being
// written behind the compiler's back. Nothing in the language stops a
// future compiler from copying or spilling it in that window (it would
// read stale data, with no fault). Today's gfx950 code touches no
// destination between issue and wait and has no scratch; re-read the
// generated code (--save-temps, -Rpass-analysis=kernel-resource-usage)
// after a compiler update or any change to the loop below
// (tests/test_wrw_halo_maps.py fails the build's suite on any scratch).
#define WH_TR(dst, addr, imm)                                   \
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"            \
               : "=v"(dst)                                      \
               : "v"(addr), "n"(imm)                            \
               : "memory")

// one k-step's operand fragments: dy for the 4 o blocks, x for every tap
template <int KYX>
struct WhFrag {
  wh_s16x4 alo[4], ahi[4], blo[KYX], bhi[KYX];
};

template <int KH, int KW>
__global__ __launch_bounds__(WH_THREADS) void conv_wrw_halo_kernel(
    const __bf16* __restrict__ dy,  // (N*H*W, Cout)
    const __bf16* __restrict__ x,   // (N, H, W, ld_x)
    const __bf16* __restrict__ x2,  // second source or nullptr
    float* __restrict__ partials,   // (nchunk, KYX, tiles_o*64, cpad)
    float* __restrict__ biasp,      // (nchunk, tiles_o*64) or nullptr
    const __bf16* __restrict__ zpage,
    int N, int H, int W, int ld_x, int ld_x2, int C1, int Cin, int Cout,
    int cpad, int tiles_o, int ntx, int nty, int nchunk, int accumulate) {
  constexpr int KYX = KH * KW;
  constexpr int LW = (WH_TW + KW - 1 + 7) / 8 * 8;
  constexpr int XP = (WH_TH + KH - 1) * LW * 8;
  constexpr int BUF = WH_DY_BYTES + XP * 16;  // one (dy, x) image pair
  __shared__ __attribute__((aligned(16))) char lds[2 * BUF];

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int to = blockIdx.x % tiles_o;
  const int tc = blockIdx.x / tiles_o;
  const int chunk = blockIdx.y;
  const int o0 = to * 64, c0 = tc * 64;

  const long ptiles = (long)N * nty * ntx;
  const int t0 = (int)((ptiles * chunk) / nchunk);
  const int t1 = (int)((ptiles * (chunk + 1)) / nchunk);

  f32x4 acc[KYX][4];
#pragma unroll
  for (int t = 0; t < KYX; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[t][i] = {0.f, 0.f, 0.f, 0.f};

  // bias gradient: every wave holds all dy fragments of the pixel tile;
  // wave 0 of the tc == 0 workgroups sums them as they pass
  const bool do_bias = biasp != nullptr && tc == 0 && wave == 0;
  float bacc[4] = {0.f, 0.f, 0.f, 0.f};

  const WhLane L = wh_lane_init(lane, wave);
  const unsigned lds0 =
      (unsigned)(unsigned long)((__attribute__((address_space(3))) char*)lds);
  const WhStage S = wh_stage_init(threadIdx.x, KW);
  // C1 % 64 == 0: this workgroup's 64-channel slab has one source tensor
  const bool from2 = x2 != nullptr && c0 >= C1;
  const __bf16* const xs = from2 ? x2 : x;
  const int xld = from2 ? ld_x2 : ld_x;
  const int cbase = from2 ? c0 - C1 : c0;

  auto stage = [&](int t, char* dimg, char* ximg) {
    const int txi = t % ntx;
    const int r = t / ntx;
    const int tyi = r % nty;
    const int n = r / nty;
    const int x0 = txi * WH_TW, y0 = tyi * WH_TH;

#pragma unroll
    for (int j = 0; j < WH_DY_PIECES / WH_THREADS; ++j) {
      const int piece0 = wave * 64 + WH_THREADS * j;
      const long off = wh_dy_src_thr(S, j, n, y0, x0, H, W, Cout, o0);
      const __bf16* src = off < 0 ? zpage : dy + off;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)src,
          (__attribute__((address_space(3))) void*)(dimg + piece0 * 16), 16,
          0, 0);
    }
    int px = S.px0, py = S.py0;
#pragma unroll 1
    for (int piece0 = wave * 64; piece0 < XP; piece0 += WH_THREADS) {
      const long off = wh_x_src_thr(S, px, py, n, y0, x0, H, W, KH, KW, xld,
                                    cbase, c0, Cin);
      const __bf16* src = off < 0 ? zpage : xs + off;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)src,
          (__attribute__((address_space(3))) void*)(ximg + piece0 * 16), 16,
          0, 0);
      wh_x_step(px, py, KW);
    }
  };

  // double-buffered pixel-tile loop: tile t+1 is staged into the other
  // image pair while tile t's MFMAs run. One barrier per tile: past it
  // every wave's pieces of tile t have landed (each waited on its own
  // loads) and every wave is done reading tile t-1, whose images the
  // staging below overwrites.
  if (t0 < t1) stage(t0, lds, lds + WH_DY_BYTES);
  int cur = 0;
  for (int t = t0; t < t1; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t + 1 < t1)
      stage(t + 1, lds + (cur ^ 1) * BUF, lds + (cur ^ 1) * BUF + WH_DY_BYTES);

    // k-step ks contracts tile row ks. The workgroup is alone on its CU
    // (LDS), so registers are plentiful and LDS latency has no second wave
    // to hide behind: all 8 + 2*KYX fragment reads of k-step ks+1 are
    // issued before the 4*KYX MFMAs of k-step ks and waited for after
    // them. Fully unrolled, every (ks, h, tap) offset is a ds_read
    // immediate on 4 + KW per-tile base registers.
    unsigned da[4], xa[KW];
#pragma unroll
    for (int i = 0; i < 4; ++i) da[i] = lds0 + (unsigned)cur * BUF + L.dy[i];
#pragma unroll
    for (int kx = 0; kx < KW; ++kx)
      xa[kx] = lds0 + (unsigned)cur * BUF + WH_DY_BYTES + L.x[kx];

    WhFrag<KYX> F[2];
    auto issue = [&](WhFrag<KYX>& f, int ks) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        WH_TR(f.alo[i], da[i], wh_dy_kstep(ks) + wh_dy_imm(0));
        WH_TR(f.ahi[i], da[i], wh_dy_kstep(ks) + wh_dy_imm(1));
      }
#pragma unroll
      for (int tap = 0; tap < KYX; ++tap) {
        const int ky = tap / KW, kx = tap % KW;
        WH_TR(f.blo[tap], xa[kx], wh_x_kstep(ks, KW) + wh_x_imm(0, ky, KW));
        WH_TR(f.bhi[tap], xa[kx], wh_x_kstep(ks, KW) + wh_x_imm(1, ky, KW));
      }
    };
    // hipcc does not track asm loads: drain lgkm, then tie every
    // destination so no use is scheduled above the wait
    auto landed = [&](WhFrag<KYX>& f) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int i = 0; i < 4; ++i)
        asm volatile("" : "+v"(f.alo[i]), "+v"(f.ahi[i]));
#pragma unroll
      for (int tap = 0; tap < KYX; ++tap)
        asm volatile("" : "+v"(f.blo[tap]), "+v"(f.bhi[tap]));
    };
    issue(F[0], 0);
    landed(F[0]);
#pragma unroll
    for (int ks = 0; ks < WH_TH; ++ks) {
      WhFrag<KYX>& f = F[ks & 1];
      if (ks + 1 < WH_TH) issue(F[(ks + 1) & 1], ks + 1);
      __builtin_amdgcn_sched_barrier(0);
      bf16x8 af[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        af[i] = __builtin_bit_cast(
            bf16x8, __builtin_shufflevector(f.alo[i], f.ahi[i], 0, 1, 2, 3, 4,
                                            5, 6, 7));
      if (do_bias) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int e = 0; e < 8; ++e) bacc[i] += (float)af[i][e];
      }
#pragma unroll
      for (int tap = 0; tap < KYX; ++tap) {
        const bf16x8 bfr = __builtin_bit_cast(
            bf16x8, __builtin_shufflevector(f.blo[tap], f.bhi[tap], 0, 1, 2,
                                            3, 4, 5, 6, 7));
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[tap][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[i], bfr, acc[tap][i], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (ks + 1 < WH_TH) landed(F[(ks + 1) & 1]);
    }
    cur ^= 1;
  }

  // partial tile: partials[chunk][tap][o0 + ..][c0 + wave*16 + ..].
  // accumulate: add to the slot this thread alone owns (see the generic
  // kernel's epilogue) instead of overwriting it
  const int orows = tiles_o * 64;
  const int fcol = lane & 15;
  const int frow0 = (lane >> 4) * 4;
#pragma unroll
  for (int tap = 0; tap < KYX; ++tap) {
    float* pbase = partials + (((long)chunk * KYX + tap) * orows) * cpad;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int o = o0 + i * 16 + frow0 + rr;
        const int c = c0 + wave * 16 + fcol;
        float v = acc[tap][i][rr];
        if (accumulate) v += pbase[(long)o * cpad + c];
        pbase[(long)o * cpad + c] = v;
      }
  }

  if (do_bias) {
    // a-fragment lane l holds o = l & 15; the four lane groups hold
    // disjoint pixel runs — fold them, lanes < 16 own the chunk's sums
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s = bacc[i];
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (lane < 16) {
        float* bp = biasp + (long)chunk * orows + o0 + i * 16 + lane;
        if (accumulate) s += *bp;
        *bp = s;
      }
    }
  }
}

// Launches the partials kernel only; the caller runs the shared reduce.
// Returns false (nothing launched) outside the envelope.
bool flowhip_conv_wrw_halo_launch(const void* dy, const void* x,
                                  const void* x2, float* partials,
                                  float* biasp, const void* zpage,
                                  const ConvGeom& g, int nchunk,
                                  bool accumulate, hipStream_t stream) {
  if (!g.wrw_halo_envelope()) return false;
  const int N = g.N(), tiles_o = g.tiles_o();
  const int ntx = fh_cdiv(g.WW, WH_TW), nty = fh_cdiv(g.HH, WH_TH);
  const long ptiles = (long)N * nty * ntx;
  // the chunk index is blockIdx.y
  if (nchunk < 1 || nchunk > ptiles || nchunk > 65535) return false;
  dim3 grid(tiles_o * g.tiles_c(), nchunk), block(WH_THREADS);
#define WH_LAUNCH(KHH, KWW)                                                  \
  if (g.KH == KHH && g.KW == KWW) {                                          \
    hipLaunchKernelGGL((conv_wrw_halo_kernel<KHH, KWW>), grid, block, 0,     \
                       stream, (const __bf16*)dy, (const __bf16*)x,          \
                       (const __bf16*)x2, partials, biasp,                   \
                       (const __bf16*)zpage, N, g.HH, g.WW, g.ld_x, g.ld_x2, \
                       g.C1, g.Cin, g.Cout, g.cpad, tiles_o, ntx, nty,       \
                       nchunk, accumulate ? 1 : 0);                          \
    return true;                                                             \
  }
  WH_LAUNCH(3, 3) WH_LAUNCH(1, 5) WH_LAUNCH(5, 1)
#undef WH_LAUNCH
  return false;
}
