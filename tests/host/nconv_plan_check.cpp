// Host check of the normalized-convolution family's host side
// (csrc/nconv.h): table membership, the fused backward's plan (workgroups,
// resolved strip length, partials columns) and the weight gradient's
// workgroup count, against values recorded from the functions as they
// stood before they moved into the header (their text, compiled unchanged
// into a scratch program over the same rows, printed these tables). The
// counts size the partials buffers the kernels write, so this runs without
// a GPU. No HIP: the header's launcher prototypes are fenced off for a
// plain host compiler.

#include <cstdio>

#include "nconv.h"

struct Triple { int K, Ci, Co; };

// every member among K in 1..7, Ci and Co in 1..8
static const Triple MEMBERS[] = {
    {1, 1, 1}, {1, 1, 2}, {1, 2, 1}, {1, 2, 2}, {1, 4, 2},
    {3, 1, 1}, {3, 1, 2}, {3, 1, 4}, {3, 2, 1}, {3, 2, 2}, {3, 2, 4},
    {3, 4, 2}, {3, 4, 4}, {3, 8, 2},
    {5, 1, 1}, {5, 1, 2}, {5, 1, 4}, {5, 2, 1}, {5, 2, 2}, {5, 2, 4},
    {5, 4, 2}, {5, 4, 4},
};
// the shipped NConvUNet layers and the folded decoder layer
static const Triple SHIPPED[] = {
    {5, 1, 2}, {5, 2, 2}, {3, 4, 2}, {3, 2, 2}, {1, 2, 1},
};
// must stay out: each ran, or aborted, on the retired untiled kernels
static const Triple OUTSIDE[] = {
    {3, 3, 2}, {5, 8, 2}, {3, 8, 4}, {1, 8, 1}, {7, 1, 1},
    {3, 4, 8}, {5, 4, 1}, {1, 4, 4},
};

struct PlanRow {
  const char* name;
  int N, Ci, Co, H, W, K, strip;  // strip: 0 = the plan's choice, else forced
  // expected: workgroups (0: refused), resolved strip, partials columns
  int nblocks, st, ncol;
};

static const PlanRow PLAN[] = {
    // fewer tiles than 384; around one strip unit; st clamped to 8; st above
    // the tile rows; forced strips; the flagship batch at both scales of the
    // net; accumulators in co groups; W % 4 != 0; off the table
    {"few_tiles_2to2_k3_19x68", 2, 2, 2, 19, 68, 3, 0,
     8, 1, 40},
    {"few_tiles_1to2_k5_5x8", 2, 1, 2, 5, 8, 5, 0,
     2, 1, 54},
    {"one_strip_unit_383tiles", 1, 2, 1, 16, 24512, 1, 0,
     383, 1, 4},
    {"exactly_384tiles", 1, 2, 1, 16, 24576, 1, 0,
     384, 1, 4},
    {"two_per_strip_768tiles", 3, 2, 2, 256, 1024, 5, 0,
     384, 2, 104},
    {"clamped_to_8_b8_448x1024", 8, 2, 2, 448, 1024, 5, 0,
     512, 8, 104},
    {"clamped_to_8_b12_448x1024", 12, 4, 2, 448, 1024, 3, 0,
     768, 8, 76},
    {"st_above_nty_b64_16x1024", 64, 2, 2, 16, 1024, 3, 0,
     1024, 1, 40},
    {"st_above_nty_b48_20x2048", 48, 1, 2, 20, 2048, 5, 0,
     1536, 2, 54},
    {"forced1_37x132", 2, 2, 2, 37, 132, 5, 1,
     18, 1, 104},
    {"forced2_37x132", 2, 2, 2, 37, 132, 5, 2,
     12, 2, 104},
    {"forced3_37x132", 2, 2, 2, 37, 132, 5, 3,
     6, 3, 104},
    {"forced5_above_nty_37x132", 2, 4, 2, 37, 132, 3, 5,
     6, 3, 76},
    {"auto_37x132", 2, 2, 2, 37, 132, 3, 0,
     18, 1, 40},
    {"flagship_1to2_k5", 6, 1, 2, 448, 1024, 5, 0,
     384, 7, 54},
    {"flagship_2to2_k5", 6, 2, 2, 448, 1024, 5, 0,
     384, 7, 104},
    {"flagship_half_2to2_k5", 6, 2, 2, 224, 512, 5, 0,
     672, 1, 104},
    {"flagship_4to2_k3", 6, 4, 2, 448, 1024, 3, 0,
     384, 7, 76},
    {"flagship_folded_2to2_k3", 6, 2, 2, 448, 1024, 3, 0,
     384, 7, 40},
    {"flagship_2to1_k1", 6, 2, 1, 448, 1024, 1, 0,
     384, 7, 4},
    {"flagship_forced4", 6, 2, 2, 448, 1024, 5, 4,
     672, 4, 104},
    {"flagship_forced14", 6, 2, 2, 448, 1024, 5, 14,
     192, 14, 104},
    {"grouped_4to4_k5_19x68", 2, 4, 4, 19, 68, 5, 0,
     8, 1, 408},
    {"w_mod4_18x22", 2, 2, 2, 18, 22, 3, 0,
     0, 0, 40},
    {"w_mod4_forced_18x22", 2, 2, 2, 18, 22, 3, 1,
     0, 0, 40},
    {"w_mod4_7x3", 2, 1, 2, 7, 3, 5, 0,
     0, 0, 54},
    {"off_table_3to2_k3", 2, 3, 2, 12, 16, 3, 0,
     0, 0, 58},
    {"off_table_8to2_k5", 2, 8, 2, 12, 16, 5, 0,
     0, 0, 404},
    {"off_table_1to1_k7", 2, 1, 1, 12, 16, 7, 0,
     0, 0, 51},
};

struct WrwRow { int N, H, W, Ci, nblocks; };

static const WrwRow WRW[] = {
    {2, 19, 68, 1, 4},       {2, 19, 68, 2, 4},
    {2, 19, 68, 4, 4},       {2, 19, 68, 8, 8},
    {6, 448, 1024, 1, 672},  {6, 448, 1024, 2, 960},
    {6, 448, 1024, 4, 1344}, {6, 448, 1024, 8, 2688},
    {2, 37, 132, 1, 6},      {2, 37, 132, 2, 6},
    {2, 37, 132, 4, 12},     {2, 37, 132, 8, 18},
    {1, 64, 64, 1, 1},       {1, 64, 64, 2, 2},
    {1, 64, 64, 4, 2},       {1, 64, 64, 8, 4},
    {1, 65, 68, 1, 4},       {1, 65, 68, 2, 4},
    {1, 65, 68, 4, 6},       {1, 65, 68, 8, 10},
};

template <typename T, int N>
constexpr int len(const T (&)[N]) { return N; }

static bool recorded(int K, int Ci, int Co) {
  for (const Triple& t : MEMBERS)
    if (t.K == K && t.Ci == Ci && t.Co == Co) return true;
  return false;
}

int main() {
  int fail = 0, rows = 0;

  // membership: the header's table is the recorded 22 and nothing else
  for (int K = 0; K <= 7; ++K)
    for (int Ci = 0; Ci <= 9; ++Ci)
      for (int Co = 0; Co <= 9; ++Co, ++rows) {
        const bool got = flowhip_nconv_supported(Ci, Co, K);
        const NConvGeom a{2, Ci, Co, 12, 16, K}, u{2, Ci, Co, 12, 18, K};
        if (got != recorded(K, Ci, Co) ||
            flowhip_nconv_launchable(a) != got ||
            flowhip_nconv_launchable(u)) {
          ++fail;
          printf("FAIL membership (K=%d, Ci=%d, Co=%d): supported %d\n", K,
                 Ci, Co, (int)got);
        }
      }
  if (len(MEMBERS) != 22) { ++fail; printf("FAIL: %d members\n", len(MEMBERS)); }
  for (const Triple& t : SHIPPED)
    if (!flowhip_nconv_supported(t.Ci, t.Co, t.K)) {
      ++fail;
      printf("FAIL shipped layer (K=%d, Ci=%d, Co=%d) is out\n", t.K, t.Ci,
             t.Co);
    }
  for (const Triple& t : OUTSIDE)
    if (flowhip_nconv_supported(t.Ci, t.Co, t.K)) {
      ++fail;
      printf("FAIL (K=%d, Ci=%d, Co=%d) is in\n", t.K, t.Ci, t.Co);
    }

  for (const PlanRow& r : PLAN) {
    ++rows;
    const NConvGeom g{r.N, r.Ci, r.Co, r.H, r.W, r.K};
    int st = r.strip;
    const int nblocks = flowhip_nconv_bwd_fused_plan(g, &st);
    const int ncol = flowhip_nconv_bwd_fused_ncol(g);
    // a refused geometry leaves the strip as passed
    const int want_st = r.nblocks ? r.st : r.strip;
    if (nblocks != r.nblocks || st != want_st || ncol != r.ncol ||
        (nblocks > 0) != flowhip_nconv_launchable(g)) {
      ++fail;
      printf("FAIL %s: got (%d, %d, %d), want (%d, %d, %d)\n", r.name,
             nblocks, st, ncol, r.nblocks, want_st, r.ncol);
    }
  }

  for (const WrwRow& r : WRW) {
    ++rows;
    const NConvGeom g{r.N, r.Ci, 2, r.H, r.W, 3};
    const int nblocks = flowhip_nconv_wrw_nblocks(g);
    if (nblocks != r.nblocks) {
      ++fail;
      printf("FAIL wrw_nblocks N=%d %dx%d Ci=%d: got %d, want %d\n", r.N,
             r.H, r.W, r.Ci, nblocks, r.nblocks);
    }
  }

  if (fail) {
    printf("%d of %d nconv plan rows differ\n", fail, rows);
    return 1;
  }
  printf("all %d nconv plan rows match\n", rows);
  return 0;
}
