// Host check of the weight-gradient plan (csrc/conv_gemm.h): path, split-M
// chunk count, partials-buffer size and the accumulate rule, for a table of
// shapes, against values recorded from the plan function as it stood
// before it took a ConvGeom (that function's text, compiled unchanged into
// a scratch program over the same rows, printed this table). A wrong chunk
// count or buffer size is a kernel writing past its buffer on the GPU, so
// this runs without one. No HIP: the header's launcher prototypes are
// fenced off for a plain host compiler.

#include <cstdio>
#include <cstring>

#include "conv_gemm.h"

struct Row {
  const char* name;
  // the conv as the Python bindings receive it: x (B, C1, H, W), optional
  // x2 (B, C2, H, W), dy with Cout channels, same padding, stride s
  int B, H, W, C1, C2, Cout, KH, KW, s, algo, nchunk_req, want_bias;
  // expected: path (-1: algo 1 refused), nchunk, buffer elements, accumulate
  int path, nchunk;
  long numel;
  int accumulate;
};

static const Row ROWS[] = {
    // update block at 3x56x128 (the measured shapes of the plan's rule
    // comments), auto; the same with the path forced; the encoder stages
    // of a batch-3 448x1024 step and both sides of the 672-pixel-tile
    // threshold; the shapes of tests/test_gpu_wrw_accumulate.py::CASES
    // (Cout as the kernels see it, padded to 8) under auto and every algo
    // they list; algo 1 forced outside the envelope; every nchunk clamp.
    {"ub_128to64_3x3", 3, 56, 128, 128, 0, 64, 3, 3, 1, -1, 0, 1,
     0, 29, 2139968L, 1},
    {"ub_256to2pad8_3x3", 3, 56, 128, 256, 0, 8, 3, 3, 1, -1, 0, 1,
     0, 15, 2212800L, 1},
    {"ub_256to192_3x3", 3, 56, 128, 256, 0, 192, 3, 3, 1, -1, 0, 1,
     1, 16, 7080960L, 0},
    {"ub_256to126pad128_3x3", 3, 56, 128, 256, 0, 128, 3, 3, 1, -1, 0, 1,
     1, 24, 7080960L, 0},
    {"ub_128to256_3x3", 3, 56, 128, 128, 0, 256, 3, 3, 1, -1, 0, 1,
     1, 24, 7084032L, 0},
    {"ub_324to256_1x1", 3, 56, 128, 324, 0, 256, 1, 1, 1, -1, 0, 1,
     0, 22, 2168320L, 1},
    {"ub_8to128_7x7", 3, 56, 128, 8, 0, 128, 7, 7, 1, -1, 0, 1,
     0, 6, 2409216L, 1},
    {"ub_128p256to256_1x5", 3, 56, 128, 128, 256, 256, 1, 5, 1, -1, 0, 1,
     1, 8, 3934208L, 0},
    {"ub_128p256to256_5x1", 3, 56, 128, 128, 256, 256, 5, 1, 1, -1, 0, 1,
     1, 8, 3934208L, 0},
    {"ub_128p256to128_1x5", 3, 56, 128, 128, 256, 128, 1, 5, 1, -1, 0, 1,
     1, 16, 3934208L, 0},
    {"ub_128p256to128_5x1", 3, 56, 128, 128, 256, 128, 5, 1, 1, -1, 0, 1,
     1, 16, 3934208L, 0},
    {"ub_128to64_3x3_algo0", 3, 56, 128, 128, 0, 64, 3, 3, 1, 0, 0, 0,
     0, 29, 2138112L, 1},
    {"ub_128to64_3x3_algo1", 3, 56, 128, 128, 0, 64, 3, 3, 1, 1, 0, 0,
     1, 96, 7077888L, 0},
    {"ub_256to192_3x3_algo0", 3, 56, 128, 256, 0, 192, 3, 3, 1, 0, 0, 0,
     0, 5, 2211840L, 1},
    {"ub_256to192_3x3_algo1", 3, 56, 128, 256, 0, 192, 3, 3, 1, 1, 0, 0,
     1, 16, 7077888L, 0},
    {"ub_128p256to256_1x5_algo0", 3, 56, 128, 128, 256, 256, 1, 5, 1, 0, 0, 0,
     0, 5, 2457600L, 1},
    {"ub_128p256to256_5x1_algo1", 3, 56, 128, 128, 256, 256, 5, 1, 1, 1, 0, 0,
     1, 8, 3932160L, 0},
    {"ub_324to256_1x1_algo1", 3, 56, 128, 324, 0, 256, 1, 1, 1, 1, 0, 0,
     -1, 0, 0, 0},
    {"ub_8to128_7x7_algo1", 3, 56, 128, 8, 0, 128, 7, 7, 1, 1, 0, 0,
     -1, 0, 0, 0},
    {"enc_64to64_s1_224x512", 3, 224, 512, 64, 0, 64, 3, 3, 1, -1, 0, 1,
     0, 57, 2104896L, 1},
    {"enc_64to96_s2_224x512", 3, 224, 512, 64, 0, 96, 3, 3, 2, -1, 0, 1,
     0, 29, 2141824L, 1},
    {"enc_96to96_s1_112x256", 3, 112, 256, 96, 0, 96, 3, 3, 1, -1, 0, 1,
     1, 48, 7084032L, 0},
    {"enc_96to128_s2_112x256", 3, 112, 256, 96, 0, 128, 3, 3, 2, -1, 0, 1,
     0, 15, 2213760L, 1},
    {"enc_128to128_s1_56x128", 3, 56, 128, 128, 0, 128, 3, 3, 1, -1, 0, 1,
     0, 15, 2213760L, 1},
    {"enc_96to96_648ptiles", 3, 108, 256, 96, 0, 96, 3, 3, 1, -1, 0, 1,
     0, 15, 2213760L, 1},
    {"enc_96to96_448ptiles", 2, 112, 256, 96, 0, 96, 3, 3, 1, -1, 0, 1,
     0, 15, 2213760L, 1},
    {"enc_96to96_896ptiles", 4, 112, 256, 96, 0, 96, 3, 3, 1, -1, 0, 1,
     1, 48, 7084032L, 0},
    {"enc_128to128_672ptiles", 12, 56, 128, 128, 0, 128, 3, 3, 1, -1, 0, 1,
     1, 48, 7084032L, 0},
    {"enc_128to128_616ptiles", 11, 56, 128, 128, 0, 128, 3, 3, 1, -1, 0, 1,
     0, 15, 2213760L, 1},
    {"enc_64to64_2688ptiles_1tile", 3, 224, 512, 64, 0, 64, 3, 3, 1, -1, 0, 0,
     0, 57, 2101248L, 1},
    {"floor_8to8_3x3", 1, 3, 5, 8, 0, 8, 3, 3, 1, -1, 0, 1,
     0, 1, 36928L, 1},
    {"floor_8to8_3x3_algo0", 1, 3, 5, 8, 0, 8, 3, 3, 1, 0, 0, 0,
     0, 1, 36864L, 1},
    {"floor_8to8_3x3_algo1", 1, 3, 5, 8, 0, 8, 3, 3, 1, 1, 0, 1,
     1, 1, 36928L, 0},
    {"tails_64to64_3x3", 2, 11, 37, 64, 0, 64, 3, 3, 1, -1, 0, 1,
     0, 13, 480064L, 1},
    {"tails_64to64_3x3_algo0", 2, 11, 37, 64, 0, 64, 3, 3, 1, 0, 0, 0,
     0, 13, 479232L, 1},
    {"tails_64to64_3x3_algo1", 2, 11, 37, 64, 0, 64, 3, 3, 1, 1, 0, 1,
     1, 12, 443136L, 0},
    {"ragged_72to126_3x3", 2, 11, 37, 72, 0, 128, 3, 3, 1, -1, 0, 1,
     0, 13, 1918592L, 1},
    {"ragged_72to126_3x3_algo0", 2, 11, 37, 72, 0, 128, 3, 3, 1, 0, 0, 0,
     0, 13, 1916928L, 1},
    {"ragged_72to126_3x3_algo1", 2, 11, 37, 72, 0, 128, 3, 3, 1, 1, 0, 1,
     1, 12, 1771008L, 0},
    {"flowhead_256to2_3x3", 2, 11, 37, 256, 0, 8, 3, 3, 1, -1, 0, 1,
     0, 13, 1917760L, 1},
    {"flowhead_256to2_3x3_algo0", 2, 11, 37, 256, 0, 8, 3, 3, 1, 0, 0, 0,
     0, 13, 1916928L, 1},
    {"flowhead_256to2_3x3_algo1", 2, 11, 37, 256, 0, 8, 3, 3, 1, 1, 0, 1,
     1, 12, 1770240L, 0},
    {"cat_64p40to64_1x5", 2, 11, 37, 64, 40, 64, 1, 5, 1, -1, 0, 1,
     0, 13, 533312L, 1},
    {"cat_64p40to64_1x5_algo0", 2, 11, 37, 64, 40, 64, 1, 5, 1, 0, 0, 0,
     0, 13, 532480L, 1},
    {"cat_64p40to64_1x5_algo1", 2, 11, 37, 64, 40, 64, 1, 5, 1, 1, 0, 1,
     1, 12, 492288L, 0},
    {"cat_64p40to64_5x1", 2, 11, 37, 64, 40, 64, 5, 1, 1, -1, 0, 1,
     0, 13, 533312L, 1},
    {"cat_64p40to64_5x1_algo0", 2, 11, 37, 64, 40, 64, 5, 1, 1, 0, 0, 0,
     0, 13, 532480L, 1},
    {"cat_64p40to64_5x1_algo1", 2, 11, 37, 64, 40, 64, 5, 1, 1, 1, 0, 1,
     1, 12, 492288L, 0},
    {"cat_128p256to128_5x1", 2, 9, 70, 128, 256, 128, 5, 1, 1, -1, 0, 1,
     1, 16, 3934208L, 0},
    {"cat_128p256to128_5x1_algo0", 2, 9, 70, 128, 256, 128, 5, 1, 1, 0, 0, 0,
     0, 9, 2211840L, 1},
    {"cat_128p256to128_5x1_algo1", 2, 9, 70, 128, 256, 128, 5, 1, 1, 1, 0, 1,
     1, 16, 3934208L, 0},
    {"narrowed_324of328to64_3x3", 2, 11, 37, 324, 0, 64, 3, 3, 1, -1, 0, 1,
     0, 10, 2212480L, 1},
    {"narrowed_324of328to64_3x3_algo0", 2, 11, 37, 324, 0, 64, 3, 3, 1, 0, 0, 0,
     0, 10, 2211840L, 1},
    {"narrowed_324of328to64_3x3_algo1", 2, 11, 37, 324, 0, 64, 3, 3, 1, 1, 0, 1,
     1, 12, 2654976L, 0},
    {"pointwise_72to64_1x1", 2, 11, 37, 72, 0, 64, 1, 1, 1, -1, 0, 1,
     0, 13, 107328L, 1},
    {"pointwise_72to64_1x1_algo0", 2, 11, 37, 72, 0, 64, 1, 1, 1, 0, 0, 0,
     0, 13, 106496L, 1},
    {"stride2_64to72_3x3", 2, 11, 37, 64, 0, 72, 3, 3, 2, -1, 0, 1,
     0, 4, 295424L, 1},
    {"stride2_64to72_3x3_algo0", 2, 11, 37, 64, 0, 72, 3, 3, 2, 0, 0, 0,
     0, 4, 294912L, 1},
    {"convf1_8to16_7x7", 2, 11, 37, 8, 0, 16, 7, 7, 1, -1, 0, 1,
     0, 11, 2208448L, 1},
    {"convf1_8to16_7x7_algo0", 2, 11, 37, 8, 0, 16, 7, 7, 1, 0, 0, 0,
     0, 11, 2207744L, 1},
    {"pointwise_72to64_1x1_algo1", 2, 11, 37, 72, 0, 64, 1, 1, 1, 1, 0, 0,
     -1, 0, 0, 0},
    {"stride2_64to72_3x3_algo1", 2, 11, 37, 64, 0, 72, 3, 3, 2, 1, 0, 0,
     -1, 0, 0, 0},
    {"convf1_8to16_7x7_algo1", 2, 11, 37, 8, 0, 16, 7, 7, 1, 1, 0, 0,
     -1, 0, 0, 0},
    {"cat_72p40_c1_not64_algo1", 2, 11, 37, 72, 40, 64, 3, 3, 1, 1, 0, 0,
     -1, 0, 0, 0},
    {"cout_12_not8_algo1", 2, 11, 37, 64, 0, 12, 3, 3, 1, 1, 0, 0,
     -1, 0, 0, 0},
    {"halo_req_above_ptiles", 1, 3, 5, 8, 0, 8, 3, 3, 1, 1, 5, 1,
     1, 1, 36928L, 0},
    {"halo_req_above_4096", 8, 224, 512, 64, 0, 64, 3, 3, 1, 1, 5000, 1,
     1, 4096, 151257088L, 0},
    {"halo_req_kept", 3, 56, 128, 256, 0, 192, 3, 3, 1, -1, 24, 1,
     1, 24, 10621440L, 0},
    {"halo_req_below_1", 3, 56, 128, 256, 0, 192, 3, 3, 1, -1, -3, 1,
     1, 16, 7080960L, 0},
    {"halo_auto_below_1_512tiles", 1, 8, 32, 4096, 0, 512, 3, 3, 1, 1, 0, 0,
     1, 1, 18874368L, 0},
    {"generic_req_above_64", 3, 56, 128, 128, 0, 64, 3, 3, 1, 0, 100, 1,
     0, 64, 4722688L, 1},
    {"generic_req_above_mtiles", 1, 3, 5, 8, 0, 8, 3, 3, 1, 0, 4, 1,
     0, 1, 36928L, 1},
    {"generic_req_kept", 3, 56, 128, 128, 0, 64, 3, 3, 1, -1, 16, 1,
     0, 16, 1180672L, 1},
    {"generic_req_below_1", 3, 56, 128, 128, 0, 64, 3, 3, 1, 0, -2, 1,
     0, 29, 2139968L, 1},
    {"generic_auto_above_64", 3, 224, 512, 64, 0, 64, 1, 1, 1, -1, 0, 0,
     0, 64, 262144L, 1},
    {"generic_auto_above_mtiles", 1, 8, 8, 64, 0, 64, 1, 1, 1, -1, 0, 0,
     0, 1, 4096L, 1},
};

static ConvGeom geom_of(const Row& r) {
  ConvGeom g{};
  g.srcH = r.H; g.srcW = r.W;
  g.HH = (r.H + 2 * (r.KH / 2) - r.KH) / r.s + 1;
  g.WW = (r.W + 2 * (r.KW / 2) - r.KW) / r.s + 1;
  g.Mtot = (long)r.B * g.HH * g.WW;
  g.sH = g.sW = r.s;
  g.C1 = r.C1; g.Cin = r.C1 + r.C2; g.Cout = r.Cout;
  g.ld_x = r.C1; g.ld_x2 = r.C2;
  g.cpad = cg_cpad(g.Cin);
  g.KH = r.KH; g.KW = r.KW; g.padH = r.KH / 2; g.padW = r.KW / 2;
  return g;
}

int main() {
  int fail = 0;
  const int n = (int)(sizeof(ROWS) / sizeof(ROWS[0]));
  for (int i = 0; i < n; ++i) {
    const Row& r = ROWS[i];
    const ConvGeom g = geom_of(r);
    int nchunk = 0;
    const int path =
        flowhip_conv_gemm_wrw_plan(g, r.algo, r.nchunk_req, &nchunk);
    bool ok = path == r.path;
    long numel = 0;
    int acc = 0;
    if (ok && path >= 0) {
      numel = g.buffer_numel(nchunk, r.want_bias != 0);
      acc = flowhip_conv_gemm_wrw_accumulate_wins(path) ? 1 : 0;
      ok = nchunk == r.nchunk && numel == r.numel && acc == r.accumulate &&
           g.buffer_numel(nchunk, false) == g.wpartials_numel(nchunk);
    }
    if (!ok) {
      ++fail;
      printf("FAIL %s: got (%d, %d, %ld, %d), want (%d, %d, %ld, %d)\n",
             r.name, path, nchunk, numel, acc, r.path, r.nchunk, r.numel,
             r.accumulate);
    }
  }
  if (fail) {
    printf("%d of %d plan rows differ\n", fail, n);
    return 1;
  }
  printf("all %d plan rows match\n", n);
  return 0;
}
