// Host check of the index maps of the on-demand correlation lookup's
// backward (csrc/alt_corr_bwd_maps.h). It re-enacts the three pieces of
// csrc/alt_corr_bwd.hip on the CPU -- direct, tiled scatter with spill, and
// finalize -- through the header's functions, with every array access going
// through a bounds-checked accessor, and compares df1 / df2 with a plain
// loop over output taps that shares none of the header's code. Operands are
// small integers and coordinates sit on the 1/8 grid, so every sum is exact
// up to the common 1/sqrt(D) factor (applied in double on both sides; the
// bound is 1e-9 against gradients of magnitude 1-5). Coordinate sets include
// +-1e6, +-inf and NaN.

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "alt_corr_bwd_maps.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (g_fail < 20) {                                  \
        printf("FAIL %s:%d: ", __FILE__, __LINE__);       \
        printf(__VA_ARGS__);                              \
        printf("\n");                                     \
      }                                                   \
      ++g_fail;                                           \
    }                                                     \
  } while (0)

// array with checked element access; a bad index is counted and redirected
template <typename T>
struct Arr {
  std::vector<T> v;
  const char* name;
  Arr(size_t n, const char* nm) : v(n + 1, T(0)), name(nm) {}
  T& at(long i) {
    if (i < 0 || i >= (long)v.size() - 1) {
      CHECK(false, "%s index %ld outside [0, %zu)", name, i, v.size() - 1);
      return v.back();
    }
    return v[i];
  }
  size_t size() const { return v.size() - 1; }
};

static unsigned rng_state = 12345u;
static unsigned rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}
static int rnd_tri() { return (int)(rnd() % 3) - 1; }
static float rnd_eighth(float lo, float hi) {  // on the 1/8 grid
  const int n = (int)((hi - lo) * 8.0f);
  return lo + (float)(rnd() % (unsigned)(n + 1)) / 8.0f;
}

struct Case {
  int B, D, H, W, R, L, cl;
  const char* coordset;
};

struct Problem {
  int B, D, H, W, P, R, K, K2, KP, L, C, cl, ldc;
  int Hs[4], Ws[4];
  Arr<float> f1, coords, grad;
  std::vector<Arr<float>> lev;
  Problem(const Case& c)
      : B(c.B), D(c.D), H(c.H), W(c.W), P(c.H * c.W), R(c.R), K(2 * c.R + 1),
        K2(K * K), KP(K + 1), L(c.L), C(c.L * K2), cl(c.cl),
        ldc(c.cl ? (C + 7) / 8 * 8 : C), f1((size_t)B * P * D, "f1"),
        coords((size_t)B * 2 * P, "coords"),
        grad(c.cl ? (size_t)B * P * ldc : (size_t)B * C * P, "grad") {
    int h = H, w = W;
    for (int l = 0; l < L; ++l) {
      Hs[l] = h;
      Ws[l] = w;
      lev.emplace_back((size_t)B * h * w * D, "level");
      h /= 2;
      w /= 2;
    }
  }
};

static void fill(Problem& p, const char* set) {
  const float inf = std::numeric_limits<float>::infinity();
  const float nan = std::numeric_limits<float>::quiet_NaN();
  for (auto& x : p.f1.v) x = (float)rnd_tri();
  for (auto& lv : p.lev)
    for (auto& x : lv.v) x = (float)rnd_tri();
  // the NHWC pad tail holds NaN: reading it poisons the result
  for (auto& x : p.grad.v) x = nan;
  for (int b = 0; b < p.B; ++b)
    for (int i = 0; i < p.P; ++i)
      for (int ch = 0; ch < p.C; ++ch)
        p.grad.at(acb_grad_off(b, i, ch, p.P, p.C, p.cl, p.ldc)) =
            (float)rnd_tri();
  const bool smooth = set[0] != 'r';
  const bool mixed = set[0] == 'm';
  const float wild[][2] = {{1e6f, -1e6f}, {nan, 3.0f},  {4.0f, nan},
                           {inf, -inf},   {-inf, 2.0f}, {-1e6f, 1e6f},
                           {nan, nan},    {1e6f, 7.0f}};
  int nw = 0;
  for (int b = 0; b < p.B; ++b)
    for (int y = 0; y < p.H; ++y)
      for (int x = 0; x < p.W; ++x) {
        float cx, cy;
        if (smooth) {
          cx = (float)x + 2.375f + rnd_eighth(-0.5f, 0.5f);
          cy = (float)y - 1.625f + rnd_eighth(-0.5f, 0.5f);
        } else {
          cx = rnd_eighth(-6.0f, (float)p.W + 5.0f);
          cy = rnd_eighth(-6.0f, (float)p.H + 5.0f);
        }
        if (mixed && rnd() % 7 == 0) {
          cx = wild[nw % 8][0];
          cy = wild[nw % 8][1];
          ++nw;
        }
        p.coords.at(((long)b * 2 + 0) * p.P + y * p.W + x) = cx;
        p.coords.at(((long)b * 2 + 1) * p.P + y * p.W + x) = cy;
      }
}

struct Grads {
  std::vector<double> df1, df2;
};

// ---- the plain loop: per output tap, grid_sample(align_corners, zeros) ----
static Grads reference(Problem& p) {
  Grads r;
  r.df1.assign((size_t)p.B * p.P * p.D, 0.0);
  r.df2.assign((size_t)p.B * p.P * p.D, 0.0);
  const double scale = 1.0 / std::sqrt((double)p.D);
  for (int l = 0; l < p.L; ++l) {
    const int Hl = p.Hs[l], Wl = p.Ws[l];
    std::vector<double> dl((size_t)p.B * Hl * Wl * p.D, 0.0);
    for (int b = 0; b < p.B; ++b)
      for (int i = 0; i < p.P; ++i) {
        const double cx = (double)p.coords.v[((long)b * 2 + 0) * p.P + i] / (1 << l);
        const double cy = (double)p.coords.v[((long)b * 2 + 1) * p.P + i] / (1 << l);
        if (!std::isfinite(cx) || !std::isfinite(cy)) continue;
        if (std::fabs(cx) > 1e5 || std::fabs(cy) > 1e5) continue;
        for (int a = 0; a < p.K; ++a)
          for (int c = 0; c < p.K; ++c) {
            const double g = p.grad.v[acb_grad_off(
                b, i, l * p.K2 + a * p.K + c, p.P, p.C, p.cl, p.ldc)];
            const double sx = cx + (a - p.R), sy = cy + (c - p.R);
            const double fx = std::floor(sx), fy = std::floor(sy);
            for (int dy = 0; dy < 2; ++dy)
              for (int dx = 0; dx < 2; ++dx) {
                const long xx = (long)fx + dx, yy = (long)fy + dy;
                if (xx < 0 || xx >= Wl || yy < 0 || yy >= Hl) continue;
                const double w = (dx ? sx - fx : 1.0 - (sx - fx)) *
                                 (dy ? sy - fy : 1.0 - (sy - fy));
                const double dc = g * w * scale;
                const size_t cell = (((size_t)b * Hl + yy) * Wl + xx) * p.D;
                for (int d = 0; d < p.D; ++d) {
                  r.df1[((size_t)b * p.P + i) * p.D + d] +=
                      dc * p.lev[l].v[cell + d];
                  dl[cell + d] += dc * p.f1.v[((size_t)b * p.P + i) * p.D + d];
                }
              }
          }
      }
    // transpose of l rounds of floor-mode 2x2 average pooling, scatter form
    const double wgt = 1.0 / (double)(1 << (2 * l));
    for (int b = 0; b < p.B; ++b)
      for (int yl = 0; yl < Hl; ++yl)
        for (int xl = 0; xl < Wl; ++xl)
          for (int dy = 0; dy < (1 << l); ++dy)
            for (int dx = 0; dx < (1 << l); ++dx) {
              const int y = (yl << l) + dy, x = (xl << l) + dx;
              if (y >= p.H || x >= p.W) {
                CHECK(false, "pooling footprint leaves the map");
                continue;
              }
              for (int d = 0; d < p.D; ++d)
                r.df2[(((size_t)b * p.H + y) * p.W + x) * p.D + d] +=
                    wgt * dl[(((size_t)b * Hl + yl) * Wl + xl) * p.D + d];
            }
  }
  return r;
}

static float dpatch(Problem& p, Arr<float>& gs, int j, int a, const float wx[2],
                    const float wy[2]) {
  int tap[4];
  const int mask = acb_taps(j, a, p.K, tap);
  int bits = 0;
  float s = 0.0f;
  for (int k = 0; k < 4; ++k)
    if (mask >> k & 1) {
      ++bits;
      s += gs.at(tap[k]) * wy[k >> 1] * wx[k & 1];
    }
  const int want = ((j == 0 || j == p.K) ? 1 : 2) * ((a == 0 || a == p.K) ? 1 : 2);
  CHECK(bits == want, "tap count %d at (%d,%d), want %d", bits, j, a, want);
  return s;
}

// ---- direct kernel, one (pixel, level) wave at a time ----
static void emulate_direct(Problem& p, std::vector<double>& df1,
                           std::vector<Arr<double>>& acc) {
  // dpatch stays exact in float; the (inexact) scale is applied in double
  const double scale = 1.0 / std::sqrt((double)p.D);
  for (int pix = 0; pix < p.B * p.P; ++pix) {
    const int b = pix / p.P, i = pix - b * p.P;
    for (int l = 0; l < p.L; ++l) {
      const int Hl = p.Hs[l], Wl = p.Ws[l];
      const float inv = 1.0f / (float)(1 << l);
      int x0, y0;
      float wx[2], wy[2];
      acb_axis(p.coords.at(((long)b * 2 + 0) * p.P + i) * inv, Wl, p.R, &x0, &wx[0], &wx[1]);
      acb_axis(p.coords.at(((long)b * 2 + 1) * p.P + i) * inv, Hl, p.R, &y0, &wy[0], &wy[1]);
      CHECK(x0 >= -(2 * p.R + 2) && x0 <= Wl + 1, "x origin %d", x0);
      CHECK(y0 >= -(2 * p.R + 2) && y0 <= Hl + 1, "y origin %d", y0);
      const bool hits = acb_axis_hits(x0, p.K, Wl) & acb_axis_hits(y0, p.K, Hl);
      if (!hits) {
        for (int j = 0; j < p.KP; ++j)
          for (int a = 0; a < p.KP; ++a)
            CHECK(!acb_in_map(x0 + a, y0 + j, Wl, Hl),
                  "a skipped window holds an in-map cell");
        continue;
      }
      Arr<float> gs(ACB_MAX_K2 + 3, "gs");
      for (int o = 0; o < p.K2; ++o) {
        const long off = acb_grad_off(b, i, l * p.K2 + o, p.P, p.C, p.cl, p.ldc);
        gs.at(o) = p.grad.at(off);
      }
      for (int j = 0; j < p.KP; ++j)
        for (int a = 0; a < p.KP; ++a) {
          const int xx = x0 + a, yy = y0 + j;
          if (!acb_in_map(xx, yy, Wl, Hl)) continue;
          const float dp = dpatch(p, gs, j, a, wx, wy);
          if (dp == 0.0f) continue;
          const long row = (((long)b * Hl + yy) * Wl + xx) * p.D;
          for (int ch = 0; ch < p.D; ++ch) {
            df1[(size_t)pix * p.D + ch] += scale * dp * p.lev[l].at(row + ch);
            acc[l].at(row + ch) += scale * dp * p.f1.at((long)pix * p.D + ch);
          }
        }
    }
  }
}

// ---- tiled scatter kernel, one workgroup at a time, pass by pass ----
struct TileStats {
  long boxed = 0, spilled = 0;
};

static void emulate_tiled(Problem& p, std::vector<Arr<double>>& acc,
                          TileStats& st) {
  // dpatch stays exact in float; the (inexact) scale is applied in double
  const double scale = 1.0 / std::sqrt((double)p.D);
  const int box = acb_box_side(p.R);
  CHECK(box <= ACB_MAX_BOX, "box side %d", box);
  const int tiles = p.B * ((p.H + ACB_TILE - 1) / ACB_TILE) *
                    ((p.W + ACB_TILE - 1) / ACB_TILE);
  const int slices = (p.D + ACB_SLICE - 1) / ACB_SLICE;
  std::vector<char> covered((size_t)p.B * p.P, 0);
  for (int tile = 0; tile < tiles; ++tile)
    for (int l = 0; l < p.L; ++l)
      for (int sl = 0; sl < slices; ++sl) {
        const int Hl = p.Hs[l], Wl = p.Ws[l];
        int b, ty, tx;
        acb_tile_decode(tile, p.H, p.W, &b, &ty, &tx);
        CHECK(b >= 0 && b < p.B && ty < p.H && tx < p.W, "tile decode");
        int org[ACB_NPIX][2], hit[ACB_NPIX], pixi[ACB_NPIX];
        float wts[ACB_NPIX][4];
        for (int t = 0; t < ACB_NPIX; ++t) {
          const int py = ty + t / ACB_TILE, px = tx + t % ACB_TILE;
          hit[t] = 0;
          org[t][0] = org[t][1] = pixi[t] = 0;
          for (int k = 0; k < 4; ++k) wts[t][k] = 0.f;
          if (py < p.H && px < p.W) {
            const int i = py * p.W + px;
            if (l == 0 && sl == 0) {
              CHECK(!covered[(size_t)b * p.P + i], "pixel in two tiles");
              covered[(size_t)b * p.P + i] = 1;
            }
            pixi[t] = i;
            const float inv = 1.0f / (float)(1 << l);
            acb_axis(p.coords.at(((long)b * 2 + 0) * p.P + i) * inv, Wl, p.R,
                     &org[t][0], &wts[t][0], &wts[t][1]);
            acb_axis(p.coords.at(((long)b * 2 + 1) * p.P + i) * inv, Hl, p.R,
                     &org[t][1], &wts[t][2], &wts[t][3]);
            hit[t] = acb_axis_hits(org[t][0], p.K, Wl) &
                     acb_axis_hits(org[t][1], p.K, Hl);
          }
        }
        int ax = ACB_NO_ANCHOR, ay = ACB_NO_ANCHOR;
        for (int t = 0; t < ACB_NPIX; ++t)
          if (hit[t]) {
            ax = acb_anchor_fold(ax, org[t][0]);
            ay = acb_anchor_fold(ay, org[t][1]);
          }
        if (ax == ACB_NO_ANCHOR) continue;
        CHECK(ax >= 0 && ax < Wl && ay >= 0 && ay < Hl, "anchor (%d,%d)", ax, ay);
        std::vector<Arr<float>> gs;
        for (int t = 0; t < ACB_NPIX; ++t) {
          gs.emplace_back(ACB_MAX_K2, "gs");
          if (!hit[t]) continue;
          for (int o = 0; o < p.K2; ++o)
            gs[t].at(o) = p.grad.at(acb_grad_off(b, pixi[t], l * p.K2 + o, p.P,
                                                 p.C, p.cl, p.ldc));
        }
        // patch gradients in box coordinates, dpb[slot][pixel]
        Arr<float> dpb((size_t)ACB_MAX_BOX * ACB_MAX_BOX * ACB_NPIX, "dpb");
        for (int idx = 0; idx < box * box * ACB_NPIX; ++idx) {
          const int t = idx & (ACB_NPIX - 1), slot = idx / ACB_NPIX;
          const int by = slot / box, bx = slot - by * box;
          const int xx = ax + bx, yy = ay + by;
          const int a = xx - org[t][0], j = yy - org[t][1];
          float dp = 0.0f;
          if (hit[t] && a >= 0 && a < p.KP && j >= 0 && j < p.KP &&
              acb_in_map(xx, yy, Wl, Hl)) {
            CHECK(acb_box_slot(xx, yy, ax, ay, box) == slot, "box slot");
            const float wx[2] = {wts[t][0], wts[t][1]};
            const float wy[2] = {wts[t][2], wts[t][3]};
            dp = dpatch(p, gs[t], j, a, wx, wy);
            st.boxed += sl == 0 && dp != 0.0f;
          }
          dpb.at((long)slot * ACB_NPIX + t) = dp;
        }
        // box pass: wave = rows by % ACB_WAVES, one add per touched cell
        for (int wave = 0; wave < ACB_WAVES; ++wave)
          for (int by = wave; by < box; by += ACB_WAVES) {
            const int yy = ay + by;
            if (yy >= Hl) break;
            CHECK(acb_row_owner(yy, ay) == wave, "row owner of box row %d", by);
            for (int bx = 0; bx < box; ++bx) {
              const int xx = ax + bx;
              if (xx >= Wl) break;
              CHECK(acb_in_map(xx, yy, Wl, Hl), "box cell outside the map");
              const int slot = by * box + bx;
              bool any = false;
              for (int t = 0; t < ACB_NPIX; ++t)
                any |= dpb.at((long)slot * ACB_NPIX + t) != 0.0f;
              if (!any) continue;
              for (int lane = 0; lane < 64; ++lane) {
                const int ch = sl * ACB_SLICE + lane;
                if (ch >= p.D) continue;
                double v = 0.0;
                for (int t = 0; t < ACB_NPIX; ++t)
                  if (hit[t])
                    v += scale * dpb.at((long)slot * ACB_NPIX + t) *
                         p.f1.at(((long)b * p.P + pixi[t]) * p.D + ch);
                acc[l].at((((long)b * Hl + yy) * Wl + xx) * p.D + ch) += v;
              }
            }
          }
        // box rows / columns the pass above stopped at hold nothing
        for (int slot = 0; slot < box * box; ++slot)
          if (!acb_in_map(ax + slot % box, ay + slot / box, Wl, Hl))
            for (int t = 0; t < ACB_NPIX; ++t)
              CHECK(dpb.at((long)slot * ACB_NPIX + t) == 0.0f,
                    "out-of-map box cell holds a gradient");
        // spill pass: in-map positions outside the box
        for (int t = 0; t < ACB_NPIX; ++t) {
          if (!hit[t]) continue;
          const bool spill = acb_axis_spills(org[t][0], p.K, Wl, ax, box) |
                             acb_axis_spills(org[t][1], p.K, Hl, ay, box);
          const float wx[2] = {wts[t][0], wts[t][1]};
          const float wy[2] = {wts[t][2], wts[t][3]};
          for (int j = 0; j < p.KP; ++j) {
            const int yy = org[t][1] + j;
            if (yy < 0 || yy >= Hl) continue;
            const int own = acb_row_owner(yy, ay);
            CHECK(own >= 0 && own < ACB_WAVES, "row owner %d", own);
            for (int a = 0; a < p.KP; ++a) {
              const int xx = org[t][0] + a;
              if (xx < 0 || xx >= Wl) continue;
              if (acb_box_slot(xx, yy, ax, ay, box) >= 0) continue;
              CHECK(spill, "a pixel the spill pass skips has a position "
                           "outside the box");
              if (!spill) continue;
              const float dp = dpatch(p, gs[t], j, a, wx, wy);
              if (dp == 0.0f) continue;
              st.spilled += sl == 0;
              for (int lane = 0; lane < 64; ++lane) {
                const int ch = sl * ACB_SLICE + lane;
                if (ch >= p.D) continue;
                acc[l].at((((long)b * Hl + yy) * Wl + xx) * p.D + ch) +=
                    scale * dp * p.f1.at(((long)b * p.P + pixi[t]) * p.D + ch);
              }
            }
          }
        }
      }
  for (char c : covered) CHECK(c, "pixel in no tile");
}

static std::vector<double> emulate_finalize(Problem& p,
                                            std::vector<Arr<double>>& acc) {
  std::vector<double> df2((size_t)p.B * p.P * p.D, 0.0);
  for (int b = 0; b < p.B; ++b)
    for (int y = 0; y < p.H; ++y)
      for (int x = 0; x < p.W; ++x)
        for (int d = 0; d < p.D; ++d) {
          double s = 0.0, wgt = 1.0;
          for (int l = 0; l < p.L; ++l) {
            if (acb_fin_member(y, x, l, p.Hs[l], p.Ws[l]))
              s += wgt * acc[l].at((((long)b * p.Hs[l] + (y >> l)) * p.Ws[l] +
                                    (x >> l)) * p.D + d);
            wgt *= 0.25;
          }
          df2[(((size_t)b * p.H + y) * p.W + x) * p.D + d] = s;
        }
  return df2;
}

static double maxdiff(const std::vector<double>& a, const std::vector<double>& b,
                      double* amax, double* nz) {
  double m = 0.0, mx = 0.0;
  size_t n = 0;
  for (size_t i = 0; i < a.size(); ++i) {
    const double d = std::fabs(a[i] - b[i]);
    if (!(d <= m)) m = d;  // NaN propagates
    mx = std::fmax(mx, std::fabs(b[i]));
    n += b[i] != 0.0;
  }
  *amax = mx;
  *nz = (double)n / (double)a.size();
  return m;
}

static std::vector<Arr<double>> make_acc(Problem& p) {
  std::vector<Arr<double>> acc;
  for (int l = 0; l < p.L; ++l)
    acc.emplace_back((size_t)p.B * p.Hs[l] * p.Ws[l] * p.D, "accumulator");
  return acc;
}

static void run(const Case& c) {
  Problem p(c);
  fill(p, c.coordset);
  const Grads ref = reference(p);

  std::vector<double> df1((size_t)p.B * p.P * p.D, 0.0);
  auto acc_d = make_acc(p);
  emulate_direct(p, df1, acc_d);
  const auto df2_d = emulate_finalize(p, acc_d);

  auto acc_t = make_acc(p);
  TileStats st;
  emulate_tiled(p, acc_t, st);
  const auto df2_t = emulate_finalize(p, acc_t);

  double mx, nz;
  const double e1 = maxdiff(df1, ref.df1, &mx, &nz);
  CHECK(e1 <= 1e-9, "df1 differs by %g", e1);
  CHECK(nz > 0.5, "reference df1 mostly zero (%g)", nz);
  const double e2 = maxdiff(df2_d, ref.df2, &mx, &nz);
  CHECK(e2 <= 1e-9, "direct df2 differs by %g", e2);
  CHECK(nz > 0.5, "reference df2 mostly zero (%g)", nz);
  const double e3 = maxdiff(df2_t, ref.df2, &mx, &nz);
  CHECK(e3 <= 1e-9, "tiled df2 differs by %g", e3);
  if (c.coordset[0] == 's')
    CHECK(st.spilled == 0, "smooth flow spilled %ld positions", st.spilled);
  CHECK(st.boxed > 0, "nothing reached the box");
  printf("B=%d D=%d %dx%d r=%d %s %-6s: df1 %.2g, df2 direct %.2g tiled %.2g "
         "(max|df2| %.3g), boxed %ld spilled %ld\n",
         c.B, c.D, c.H, c.W, c.R, c.cl ? "nhwc" : "nchw", c.coordset, e1, e2,
         e3, mx, st.boxed, st.spilled);
}

int main() {
  const Case cases[] = {
      {2, 8, 16, 24, 4, 4, 1, "rand"},   {2, 8, 16, 24, 4, 4, 1, "smooth"},
      {2, 8, 16, 24, 4, 4, 0, "mixed"},  {1, 8, 17, 27, 3, 4, 1, "rand"},
      {1, 8, 17, 27, 3, 4, 0, "smooth"}, {1, 72, 17, 27, 3, 4, 1, "mixed"},
      {1, 8, 9, 6, 4, 3, 1, "mixed"},
  };
  for (const Case& c : cases) run(c);
  if (g_fail) {
    printf("%d address-map checks FAILED\n", g_fail);
    return 1;
  }
  printf("all address-map checks passed\n");
  return 0;
}
