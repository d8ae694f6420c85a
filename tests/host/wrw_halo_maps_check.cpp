// Host check of the halo-staged weight-gradient kernel's address maps
// (csrc/conv_wrw_halo_maps.h). For every test shape it enumerates every
// address the kernel forms and asserts
//   - every global source is inside its tensor (16-B piece) or the zero page,
//     and the per-thread form the kernel runs equals the per-piece map;
//   - every LDS address is inside its image, 16-B aligned for staging and
//     8-B aligned for transposed reads, never in a padding column, and each
//     32-lane half of a transposed read covers 64 distinct banks;
//   - emulating stage -> transposed read -> MFMA operand order reproduces the
//     dW and dbias of a direct loop exactly (small-integer bf16 data).
// Build with the host compiler; sanitizers welcome:
//   c++ -O1 -g -fsanitize=address,undefined -I csrc tests/host/wrw_halo_maps_check.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "conv_wrw_halo_maps.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (g_fail < 20) {                                   \
        printf("FAIL %s:%d %s : ", __FILE__, __LINE__, #cond); \
        printf(__VA_ARGS__);                               \
        printf("\n");                                      \
      }                                                    \
      ++g_fail;                                            \
    }                                                      \
  } while (0)

struct Shape {
  const char* name;
  int N, H, W, C1, C2, Cout, KH, KW, ldpad;  // ldpad: extra row stride of x
};

static uint16_t bf16_of_int(int v) {  // exact for |v| <= 256
  float f = (float)v;
  uint32_t u;
  memcpy(&u, &f, 4);
  return (uint16_t)(u >> 16);
}
static float f_of_bf16(uint16_t h) {
  uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static uint32_t g_rng = 12345u;
static int rnd_small() {
  g_rng = g_rng * 1664525u + 1013904223u;
  return (int)((g_rng >> 24) % 7) - 3;
}

// transposed read of one 16-lane group: lane 4q+p supplies the address of
// row q, columns 4p..4p+3; lane i receives column i, row q in element q
static void tr_read_group(const std::vector<uint16_t>& img,
                          const unsigned addr[16], uint16_t out[16][4]) {
  for (int i = 0; i < 16; ++i)
    for (int q = 0; q < 4; ++q)
      out[i][q] = img[addr[4 * q + i / 4] / 2 + (i & 3)];
}

static void check_banks(const unsigned addr[64], const char* what) {
  for (int half = 0; half < 2; ++half) {
    int seen[64] = {0};
    for (int l = half * 32; l < half * 32 + 32; ++l)
      for (int d = 0; d < 2; ++d) {
        const int bank = (addr[l] / 4 + d) % 64;
        CHECK(seen[bank] == 0, "%s bank %d twice in half %d", what, bank,
              half);
        seen[bank] = 1;
      }
  }
}

static void run_shape(const Shape& sh) {
  const int N = sh.N, H = sh.H, W = sh.W, KH = sh.KH, KW = sh.KW;
  const int Cin = sh.C1 + sh.C2, Cout = sh.Cout, KYX = KH * KW;
  const bool has2 = sh.C2 > 0;
  const int ld_x = sh.C1 + sh.ldpad, ld_x2 = sh.C2;
  const int cpad = (Cin + 63) / 64 * 64;
  const int tiles_o = (Cout + 63) / 64, tiles_c = cpad / 64;
  const int ntx = (W + WH_TW - 1) / WH_TW, nty = (H + WH_TH - 1) / WH_TH;
  const int LW = wh_lw(KW), LH = wh_lh(KH), XP = wh_x_pieces(KH, KW);
  const long npix = (long)N * H * W;
  CHECK(XP % 64 == 0, "x pieces %d", XP);

  std::vector<uint16_t> dy(npix * Cout), x(npix * ld_x),
      x2(has2 ? npix * ld_x2 : 0);
  for (auto& v : dy) v = bf16_of_int(rnd_small());
  for (auto& v : x) v = bf16_of_int(rnd_small());
  for (auto& v : x2) v = bf16_of_int(rnd_small());

  // direct reference (ints are exact in double)
  std::vector<double> ref((size_t)Cout * KYX * Cin, 0.0), refb(Cout, 0.0);
  for (int n = 0; n < N; ++n)
    for (int y = 0; y < H; ++y)
      for (int xx = 0; xx < W; ++xx) {
        const uint16_t* dp = &dy[(((long)n * H + y) * W + xx) * Cout];
        for (int o = 0; o < Cout; ++o) refb[o] += f_of_bf16(dp[o]);
        for (int ky = 0; ky < KH; ++ky)
          for (int kx = 0; kx < KW; ++kx) {
            const int sy = y + ky - KH / 2, sx = xx + kx - KW / 2;
            if (sy < 0 || sy >= H || sx < 0 || sx >= W) continue;
            const long sp = ((long)n * H + sy) * W + sx;
            for (int o = 0; o < Cout; ++o) {
              const double d = f_of_bf16(dp[o]);
              if (d == 0.0) continue;
              double* r = &ref[((size_t)o * KYX + ky * KW + kx) * Cin];
              for (int c = 0; c < Cin; ++c) {
                const uint16_t xv = c < sh.C1 ? x[sp * ld_x + c]
                                              : x2[sp * ld_x2 + (c - sh.C1)];
                r[c] += d * f_of_bf16(xv);
              }
            }
          }
      }

  // transposed-read addresses: lane maps, bounds, alignment, banks
  for (int ks = 0; ks < WH_TH; ++ks)
    for (int h = 0; h < 2; ++h) {
      for (int i = 0; i < 4; ++i) {
        unsigned a[64];
        for (int lane = 0; lane < 64; ++lane) {
          const WhLane L = wh_lane_init(lane, 0);
          a[lane] = wh_dy_addr(L, ks, h, i);
          CHECK(a[lane] == wh_tr_addr(wh_dy_pix(ks, wh_tr_tx(lane, h)), i,
                                      lane),
                "dy tr addr lane %d", lane);
          CHECK(a[lane] % 8 == 0 && a[lane] + 8 <= WH_DY_BYTES,
                "dy tr addr %u", a[lane]);
        }
        check_banks(a, "dy");
      }
      for (int cb = 0; cb < 4; ++cb)
        for (int tap = 0; tap < KYX; ++tap) {
          const int ky = tap / KW, kx = tap % KW;
          unsigned a[64];
          for (int lane = 0; lane < 64; ++lane) {
            const WhLane L = wh_lane_init(lane, cb);
            a[lane] = wh_x_addr(L, ks, h, ky, kx, KW);
            const int tx = wh_tr_tx(lane, h);
            CHECK(a[lane] == wh_tr_addr(wh_x_pix(ks, tx, ky, kx, KW), cb,
                                        lane),
                  "x tr addr lane %d tap %d", lane, tap);
            CHECK(a[lane] % 8 == 0 && a[lane] + 8 <= (unsigned)XP * 16,
                  "x tr addr %u", a[lane]);
            CHECK(tx + kx < WH_TW + KW - 1 && ks + ky < LH,
                  "x tr read in padding");
          }
          check_banks(a, "x");
        }
    }

  // staging + emulated MFMA per output tile
  std::vector<double> got((size_t)Cout * KYX * Cin, 0.0), gotb(Cout, 0.0);
  std::vector<uint16_t> dimg(WH_DY_BYTES / 2), ximg((size_t)XP * 8);
  for (int to = 0; to < tiles_o; ++to)
    for (int tc = 0; tc < tiles_c; ++tc) {
      const int o0 = to * 64, c0 = tc * 64;
      const bool from2 = has2 && c0 >= sh.C1;
      const std::vector<uint16_t>& xs = from2 ? x2 : x;
      const int xld = from2 ? ld_x2 : ld_x;
      const int cbase = from2 ? c0 - sh.C1 : c0;
      std::vector<double> acc((size_t)KYX * 64 * 64, 0.0);
      double bsum[64] = {0};
      for (int n = 0; n < N; ++n)
        for (int tyi = 0; tyi < nty; ++tyi)
          for (int txi = 0; txi < ntx; ++txi) {
            const int y0 = tyi * WH_TH, x0 = txi * WH_TW;
            // poison: a piece the staging skips would show up
            std::fill(dimg.begin(), dimg.end(), bf16_of_int(100));
            std::fill(ximg.begin(), ximg.end(), bf16_of_int(100));
            for (int tid = 0; tid < WH_THREADS; ++tid) {
              const WhStage S = wh_stage_init(tid, KW);
              for (int j = 0; j < WH_DY_PIECES / WH_THREADS; ++j) {
                const int piece = tid + WH_THREADS * j;
                const long off =
                    wh_dy_src_thr(S, j, n, y0, x0, H, W, Cout, o0);
                CHECK(off == wh_dy_src(piece, n, y0, x0, H, W, Cout, o0),
                      "dy src tid %d j %d", tid, j);
                CHECK(piece * 16 + 16 <= WH_DY_BYTES, "dy lds piece %d",
                      piece);
                if (off >= 0) {
                  CHECK(off % 8 == 0 && off + 8 <= npix * Cout,
                        "dy src off %ld", off);
                  if (off + 8 <= npix * Cout)
                    memcpy(&dimg[piece * 8], &dy[off], 16);
                } else {
                  memset(&dimg[piece * 8], 0, 16);
                }
              }
              int px = S.px0, py = S.py0;
              for (int piece = tid; piece < XP; piece += WH_THREADS) {
                const long off = wh_x_src_thr(S, px, py, n, y0, x0, H, W, KH,
                                              KW, xld, cbase, c0, Cin);
                int which;
                const long off0 =
                    wh_x_src(piece, n, y0, x0, H, W, KH, KW, ld_x, ld_x2,
                             sh.C1, Cin, has2, c0, &which);
                CHECK((which == 0) == (off < 0), "x src zero piece %d", piece);
                if (which != 0) {
                  CHECK(off == off0 && (which == 2) == from2,
                        "x src piece %d: %ld vs %ld", piece, off, off0);
                  const long lim = npix * xld;
                  CHECK(off >= 0 && off + 8 <= lim, "x src off %ld", off);
                  if (off >= 0 && off + 8 <= lim)
                    memcpy(&ximg[(size_t)piece * 8], &xs[off], 16);
                } else {
                  memset(&ximg[(size_t)piece * 8], 0, 16);
                }
                wh_x_step(px, py, KW);
              }
              // after the last piece the walk has covered the whole image
            }
            // compute: 4 waves, wave w owns c block w
            for (int ks = 0; ks < WH_TH; ++ks)
              for (int w = 0; w < 4; ++w) {
                // A fragments: a[i][lane][e]
                static uint16_t af[4][64][8], bfv[64][8];
                for (int i = 0; i < 4; ++i)
                  for (int h = 0; h < 2; ++h)
                    for (int g = 0; g < 4; ++g) {
                      unsigned a[16];
                      uint16_t out[16][4];
                      for (int l = 0; l < 16; ++l)
                        a[l] = wh_dy_addr(wh_lane_init(g * 16 + l, w), ks, h,
                                          i);
                      tr_read_group(dimg, a, out);
                      for (int l = 0; l < 16; ++l)
                        for (int q = 0; q < 4; ++q)
                          af[i][g * 16 + l][h * 4 + q] = out[l][q];
                    }
                if (w == 0 && tc == 0)
                  for (int i = 0; i < 4; ++i)
                    for (int lane = 0; lane < 64; ++lane)
                      for (int e = 0; e < 8; ++e)
                        bsum[i * 16 + (lane & 15)] +=
                            f_of_bf16(af[i][lane][e]);
                for (int tap = 0; tap < KYX; ++tap) {
                  const int ky = tap / KW, kx = tap % KW;
                  for (int h = 0; h < 2; ++h)
                    for (int g = 0; g < 4; ++g) {
                      unsigned a[16];
                      uint16_t out[16][4];
                      for (int l = 0; l < 16; ++l)
                        a[l] = wh_x_addr(wh_lane_init(g * 16 + l, w), ks, h,
                                         ky, kx, KW);
                      tr_read_group(ximg, a, out);
                      for (int l = 0; l < 16; ++l)
                        for (int q = 0; q < 4; ++q)
                          bfv[g * 16 + l][h * 4 + q] = out[l][q];
                    }
                  // MFMA 16x16x32: A[row = lane&15][k = (lane>>4)*8 + e],
                  // B[k = (lane>>4)*8 + e][col = lane&15]
                  for (int i = 0; i < 4; ++i)
                    for (int la = 0; la < 64; ++la)
                      for (int e = 0; e < 8; ++e) {
                        const double av = f_of_bf16(af[i][la][e]);
                        if (av == 0.0) continue;
                        const int row = la & 15, g = la >> 4;
                        for (int col = 0; col < 16; ++col)
                          acc[((size_t)tap * 64 + i * 16 + row) * 64 +
                              w * 16 + col] +=
                              av * f_of_bf16(bfv[g * 16 + col][e]);
                      }
                }
              }
          }
      for (int tap = 0; tap < KYX; ++tap)
        for (int o = 0; o < 64 && o0 + o < Cout; ++o)
          for (int c = 0; c < 64 && c0 + c < Cin; ++c)
            got[((size_t)(o0 + o) * KYX + tap) * Cin + c0 + c] =
                acc[((size_t)tap * 64 + o) * 64 + c];
      if (tc == 0)
        for (int o = 0; o < 64 && o0 + o < Cout; ++o) gotb[o0 + o] = bsum[o];
    }
  long bad = 0;
  for (size_t k = 0; k < ref.size(); ++k) bad += ref[k] != got[k];
  CHECK(bad == 0, "%s: %ld dW elements differ", sh.name, bad);
  long badb = 0;
  for (int o = 0; o < Cout; ++o) badb += refb[o] != gotb[o];
  CHECK(badb == 0, "%s: %ld dbias elements differ", sh.name, badb);

  // chunk count: never more chunks than pixel tiles, never zero
  const long ptiles = (long)N * nty * ntx;
  const int nch = wh_nchunk(ptiles, tiles_o * tiles_c);
  CHECK(nch >= 1 && nch <= ptiles, "nchunk %d of %ld", nch, ptiles);
  printf("%-30s ok=%d  ptiles=%ld tiles=%d nchunk=%d\n", sh.name,
         bad == 0 && badb == 0, ptiles, tiles_o * tiles_c, nch);
}

int main() {
  // the cases of tests/test_gpu_wrw_halo.py (Cout already padded to 8 the
  // way the autograd functions pad dy)
  const Shape shapes[] = {
      {"floor 1x3x5 8->8 3x3", 1, 3, 5, 8, 0, 8, 3, 3, 0},
      {"tails 2x11x37 64->64 3x3", 2, 11, 37, 64, 0, 64, 3, 3, 0},
      {"ragged 72->126(128) 3x3", 2, 11, 37, 72, 0, 128, 3, 3, 0},
      {"flow head 256->2(8) 3x3", 2, 11, 37, 256, 0, 8, 3, 3, 0},
      {"two-source 64+40->64 1x5", 2, 11, 37, 64, 40, 64, 1, 5, 0},
      {"two-source 64+40->64 5x1", 2, 11, 37, 64, 40, 64, 5, 1, 0},
      {"two-source 128+256->128 5x1", 2, 9, 70, 128, 256, 128, 5, 1, 0},
      {"narrowed 324 of 328 ->64 3x3", 2, 11, 37, 324, 0, 64, 3, 3, 4},
  };
  for (const Shape& s : shapes) run_shape(s);
  if (g_fail) {
    printf("%d checks FAILED\n", g_fail);
    return 1;
  }
  printf("all address-map checks passed\n");
  return 0;
}
