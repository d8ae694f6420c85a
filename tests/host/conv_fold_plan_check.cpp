// Host check of the tap-folded conv path (csrc/conv_fold.h): the envelope,
// the weight-gradient plan and the index maps the kernels of conv_gemm.hip
// run, by brute-force enumeration and not from recorded numbers. For every
// row of the table:
//   - every (o, c, ky, kx) maps to exactly one in-range element of the
//     folded pack and one of dw, and the pack kernel's decode inverts it;
//   - in both ky forms, every partials slot the reduce reads is written by
//     exactly one (workgroup, thread) of the planned grid, no slot is
//     written twice, every write is inside the buffer, and the buffer size
//     is the largest index + 1 (bias tail included);
//   - the chunks' m-tile ranges partition the m-tiles.
// A wrong map is a kernel writing past its buffer on the GPU, so this runs
// without one. No HIP: the launcher prototypes are fenced off.

#include <cstdio>
#include <vector>

#include "conv_fold.h"

static int fails = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      ++fails;                               \
      std::printf("FAIL %s: ", row_name);    \
      std::printf(__VA_ARGS__);              \
      std::printf("\n");                     \
    }                                        \
  } while (0)

// a conv as the bindings build it: x (B, 8, H, W) with row stride ld,
// same padding, stride s, dy with Cout channels
static ConvGeom geom(int B, int H, int W, int Cout, int KH, int KW, int s,
                     int ld = 8) {
  ConvGeom g{};
  g.srcH = H; g.srcW = W;
  g.C1 = g.Cin = 8; g.cpad = cg_cpad(8);
  g.ld_x = ld;
  g.KH = KH; g.KW = KW; g.padH = KH / 2; g.padW = KW / 2;
  g.sH = g.sW = s;
  g.HH = s == 1 ? H : (H + 2 * g.padH - KH) / s + 1;
  g.WW = s == 1 ? W : (W + 2 * g.padW - KW) / s + 1;
  g.Cout = Cout;
  g.Mtot = (long)B * g.HH * g.WW;
  return g;
}

struct Row {
  const char* name;
  int B, H, W, Cout, KH, KW, s, nchunk_req;
};

static const Row ROWS[] = {
    // the flagship layers: both encoder stems and convf1
    {"stem_fnet_b6", 6, 448, 1024, 64, 7, 7, 2, 0},
    {"stem_cnet_b3", 3, 448, 1024, 64, 7, 7, 2, 0},
    {"convf1_b3", 3, 56, 128, 128, 7, 7, 1, 0},
    // the GPU tests' shapes: ragged Cout below one N tile, odd stride-2
    {"edges_2x11x37_to16", 2, 11, 37, 16, 7, 7, 1, 0},
    {"stride2_odd_23x37", 2, 23, 37, 64, 7, 7, 2, 0},
    {"stride2_30x48", 2, 30, 48, 64, 7, 7, 2, 0},
    {"kh1", 2, 24, 40, 16, 1, 7, 1, 0},
    {"kw1", 2, 24, 40, 16, 7, 1, 1, 0},
    {"kw3", 2, 24, 40, 16, 3, 3, 1, 0},
    {"kw8_ragged_cout72", 1, 9, 20, 72, 3, 8, 1, 0},
    // forced chunk counts at both clamps
    {"convf1_b3_n1", 3, 56, 128, 128, 7, 7, 1, 1},
    {"convf1_b3_nmax", 3, 56, 128, 128, 7, 7, 1, 1000000},
    {"stem_cnet_b3_nmax", 3, 448, 1024, 64, 7, 7, 2, 1000000},
    {"edges_n1", 2, 11, 37, 16, 7, 7, 1, 1},
    {"edges_nmax", 2, 11, 37, 16, 7, 7, 1, 1000000},
};

static void check_maps(const char* row_name, const ConvGeom& g) {
  const int O = g.Cout, KH = g.KH, KW = g.KW;
  const long npack = (long)KH * O * 64, ndw = (long)O * 8 * KH * KW;
  std::vector<unsigned char> pack(npack, 0), dw(ndw, 0);
  for (int o = 0; o < O; ++o)
    for (int c = 0; c < 8; ++c)
      for (int ky = 0; ky < KH; ++ky)
        for (int kx = 0; kx < KW; ++kx) {
          const long p = cf_pack_index(ky, o, kx, c, O);
          const long d = cf_dw_index(o, c, ky, kx, 8, KH, KW);
          CHECK(p >= 0 && p < npack, "pack index %ld out of range", p);
          CHECK(d >= 0 && d < ndw, "dw index %ld out of range", d);
          if (p < 0 || p >= npack || d < 0 || d >= ndw) return;
          ++pack[p];
          ++dw[d];
          // the pack kernel's decode of a flat index (conv_gemm_pack_kernel)
          const int col = (int)(p % 64), r = (int)((p / 64) % O),
                    t = (int)(p / 64 / O);
          CHECK(t == ky && r == o && (col >> 3) == kx && (col & 7) == c,
                "pack decode of %ld", p);
        }
  long pack_hit = 0;
  for (long i = 0; i < npack; ++i) {
    CHECK(pack[i] <= 1, "pack element %ld hit %d times", i, pack[i]);
    pack_hit += pack[i];
  }
  CHECK(pack_hit == ndw, "pack hits %ld", pack_hit);
  for (long i = 0; i < ndw; ++i)
    CHECK(dw[i] == 1, "dw element %ld hit %d times", i, dw[i]);
}

static void check_form(const char* row_name, const ConvGeom& g, int form_req,
                       int nchunk_req) {
  int nchunk = 0;
  const int form = flowhip_conv_fold_wrw_plan(g, form_req, nchunk_req,
                                              &nchunk);
  CHECK(form == form_req, "form %d for request %d", form, form_req);
  int auto_n = 0;
  CHECK(flowhip_conv_fold_wrw_plan(g, -1, nchunk_req, &auto_n) == 0,
        "the rule keeps ky in the grid");
  const long mtiles = (g.Mtot + 63) / 64;
  CHECK(nchunk >= 1 && nchunk <= mtiles && nchunk <= 4096, "nchunk %d",
        nchunk);
  if (nchunk_req == 1) CHECK(nchunk == 1, "nchunk %d at the low clamp", nchunk);
  if (nchunk_req > 4096)
    CHECK(nchunk == (mtiles < 4096 ? mtiles : 4096),
          "nchunk %d at the high clamp", nchunk);
  // a planned count is a fixed point of the plan (the bindings re-plan)
  int again = 0;
  flowhip_conv_fold_wrw_plan(g, form_req, nchunk, &again);
  CHECK(again == nchunk, "re-planned %d != %d", again, nchunk);

  // the chunks' m-tile ranges partition [0, mtiles)
  long next = 0;
  for (int ch = 0; ch < nchunk; ++ch) {
    const long t0 = (mtiles * ch) / nchunk, t1 = (mtiles * (ch + 1)) / nchunk;
    CHECK(t0 == next && t1 > t0, "chunk %d walks [%ld, %ld)", ch, t0, t1);
    next = t1;
  }
  CHECK(next == mtiles, "chunks end at %ld of %ld", next, mtiles);

  const int tiles_o = g.tiles_o(), orows = tiles_o * 64, KH = g.KH;
  const long nw = cf_wpartials_numel(g, nchunk);
  const long nb = (long)nchunk * orows;
  const long numel = cf_buffer_numel(g, nchunk, true);
  CHECK(numel == nw + nb, "buffer %ld != %ld + %ld", numel, nw, nb);
  CHECK(cf_buffer_numel(g, nchunk, false) == nw, "buffer without bias");
  std::vector<unsigned char> hits(numel, 0);
  long largest = -1;
  for (int bz = 0; bz < nchunk; ++bz)
    for (int by = 0; by < cf_grid_y(g, form); ++by)
      for (int bx = 0; bx < tiles_o; ++bx)
        for (int tid = 0; tid < 256; ++tid) {
          const int wave = tid >> 6, lane = tid & 63, o0 = bx * 64;
          const int ky0 = cf_ky0(form, by), nky = cf_nky(form, KH);
          for (int k = 0; k < nky; ++k)
            for (int i = 0; i < 2; ++i)
              for (int j = 0; j < 2; ++j)
                for (int r = 0; r < 4; ++r) {
                  const long s = cf_partial_index(
                      bz, ky0 + k, o0 + cf_acc_orow(wave, lane, i, r),
                      cf_acc_col(wave, lane, j), KH, orows);
                  if (s < 0 || s >= nw) {
                    CHECK(false, "weight slot %ld outside [0, %ld)", s, nw);
                    return;
                  }
                  ++hits[s];
                  if (s > largest) largest = s;
                }
          // bias partials: even waves (column offset 0) of the ky == 0
          // workgroups, lanes < 16
          if (ky0 == 0 && (wave & 1) == 0 && lane < 16)
            for (int i = 0; i < 2; ++i) {
              const long s = nw + cf_bias_index(
                  bz, o0 + cf_bias_orow(wave, lane, i), orows);
              if (s < nw || s >= numel) {
                CHECK(false, "bias slot %ld outside the tail", s);
                return;
              }
              ++hits[s];
              if (s > largest) largest = s;
            }
        }
  CHECK(largest + 1 == numel, "largest index %ld, buffer %ld", largest,
        numel);
  long twice = 0;
  for (long s = 0; s < numel; ++s) twice += hits[s] > 1;
  CHECK(twice == 0, "%ld slots have more than one owner", twice);
  // what the reduce reads (conv_wrw_fold_reduce_kernel)
  long unwritten = 0;
  for (int ch = 0; ch < nchunk; ++ch) {
    for (int ky = 0; ky < KH; ++ky)
      for (int o = 0; o < g.Cout; ++o)
        for (int col = 0; col < g.KW * 8; ++col)
          unwritten += hits[cf_partial_index(ch, ky, o, col, KH, orows)] != 1;
    for (int o = 0; o < g.Cout; ++o)
      unwritten += hits[nw + cf_bias_index(ch, o, orows)] != 1;
  }
  CHECK(unwritten == 0, "%ld slots the reduce reads lack their one writer",
        unwritten);
}

int main() {
  const char* row_name = "envelope";
  // the three flagship layers are inside
  CHECK(flowhip_conv_fold_envelope(geom(6, 448, 1024, 64, 7, 7, 2)), "fnet");
  CHECK(flowhip_conv_fold_envelope(geom(3, 448, 1024, 64, 7, 7, 2)), "cnet");
  CHECK(flowhip_conv_fold_envelope(geom(3, 56, 128, 128, 7, 7, 1)), "convf1");
  CHECK(flowhip_conv_fold_wrw_envelope(geom(3, 56, 128, 128, 7, 7, 1)),
        "convf1 wrw");
  {
    ConvGeom g = geom(3, 56, 128, 128, 7, 7, 1);
    g.Cin = 16;  // a second source: channels [8, 16) from x2
    CHECK(g.two_source() && !flowhip_conv_fold_envelope(g), "second source");
    g = geom(3, 56, 128, 128, 7, 7, 1);
    g.C1 = g.Cin = 16;
    CHECK(!flowhip_conv_fold_envelope(g), "Cin 16");
    g.C1 = g.Cin = 4;
    CHECK(!flowhip_conv_fold_envelope(g), "Cin 4");
    CHECK(!flowhip_conv_fold_envelope(geom(3, 56, 128, 128, 7, 9, 1)), "KW 9");
    g = geom(3, 56, 128, 128, 7, 7, 1);
    g.padH = 2;
    CHECK(!flowhip_conv_fold_envelope(g), "padH 2 of a 7-row kernel");
    g = geom(3, 56, 128, 128, 7, 7, 1);
    g.padW = 0;
    CHECK(!flowhip_conv_fold_envelope(g), "padW 0");
    CHECK(!flowhip_conv_fold_envelope(geom(3, 56, 128, 128, 7, 7, 3)),
          "stride 3");
    CHECK(!flowhip_conv_fold_envelope(geom(3, 56, 128, 128, 7, 7, 1, 12)),
          "row stride 12");
    CHECK(flowhip_conv_fold_envelope(geom(3, 56, 128, 128, 7, 7, 1, 16)),
          "row stride 16");
    g = geom(3, 56, 128, 12, 7, 7, 1);
    CHECK(flowhip_conv_fold_envelope(g) && !flowhip_conv_fold_wrw_envelope(g),
          "Cout 12: forward only");
    int n = 0;
    CHECK(flowhip_conv_fold_wrw_plan(geom(2, 24, 40, 16, 9, 1, 1), 1, 0,
                                     &n) == -1, "looped form with KH 9");
  }
  // the rule: ky in the grid; two workgroups per CU on the stems, 16
  // m-tiles per workgroup on convf1
  {
    int n = 0;
    CHECK(flowhip_conv_fold_wrw_plan(geom(6, 448, 1024, 64, 7, 7, 2), -1, 0,
                                     &n) == 0 && n == 74, "fnet plan %d", n);
    CHECK(flowhip_conv_fold_wrw_plan(geom(3, 448, 1024, 64, 7, 7, 2), -1, 0,
                                     &n) == 0 && n == 74, "cnet plan %d", n);
    CHECK(flowhip_conv_fold_wrw_plan(geom(3, 56, 128, 128, 7, 7, 1), -1, 0,
                                     &n) == 0 && n == 21, "convf1 plan %d", n);
    CHECK(flowhip_conv_fold_wrw_plan(geom(3, 56, 128, 128, 7, 7, 1), 1, 0,
                                     &n) == 1 && n == 128, "convf1 looped %d",
          n);
  }

  int rows = 0;
  for (const Row& r : ROWS) {
    row_name = r.name;
    const ConvGeom g = geom(r.B, r.H, r.W, r.Cout, r.KH, r.KW, r.s);
    CHECK(flowhip_conv_fold_wrw_envelope(g), "outside the envelope");
    check_maps(row_name, g);
    check_form(row_name, g, 0, r.nchunk_req);
    check_form(row_name, g, 1, r.nchunk_req);
    ++rows;
  }
  if (fails) {
    std::printf("%d check(s) failed\n", fails);
    return 1;
  }
  std::printf("conv fold maps hold for %d rows in both ky forms\n", rows);
  return 0;
}
