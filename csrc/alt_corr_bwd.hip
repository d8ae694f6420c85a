// Backward of the on-demand correlation window lookup (alt_corr.hip):
// gradients for the f1 rows and for the second feature map, with nothing of
// size P^2 alive. Index logic lives in alt_corr_bwd_maps.h (host-checked).
//
// Per (target pixel i, level l) the forward blended a (K+1)^2 patch of dot
// products <f1[i], F2_l[pos]> * scale into K^2 taps. Transposed:
//     dpatch[pos]  = scale * sum over the <= 4 taps that blended pos
//     df1[i, :]   += dpatch[pos] * F2_l[pos, :]      (in-map pos only)
//     dF2_l[pos,:]+= dpatch[pos] * f1[i, :]
// and the level gradients fold back through the floor-mode pooling chain:
//     df2[y,x] = g0[y,x] + g1[y>>1,x>>1]/4 + g2[y>>2,x>>2]/16 + g3[..]/64.
//
// Lane layout everywhere: lane = channel (ch = lane + 64 n), so one atomic
// wave-instruction adds 256 contiguous bytes of one accumulator row -- the
// shape global float atomics run at full rate for -- and df1 needs no
// cross-lane reduction.
//
// alt_corr_bwd_direct_kernel<NC, ATOMICS>: one workgroup per target pixel,
//   wave = level (64 L threads). Each wave turns its level's K^2 cotangents
//   into the patch gradient in LDS, then walks the in-map positions whose
//   dpatch is nonzero: one 2-byte-per-lane read of the F2 row per 64
//   channels feeds df1 (registers), and with ATOMICS one no-return
//   global_atomic_add_f32 per 64 channels feeds the fp32 level accumulator.
//   The level waves' df1 partials meet in LDS and the row is stored once.
//   With the atomics compiled out (ATOMICS = false: the `tiled` path's df1
//   kernel, and every f1-only call) nothing ties a lane to one channel, so
//   the lane owns channel quads instead and a row's K+1 reads, 8 bytes per
//   lane, are issued together (acb_df1_rows).
//   LDS 10.9 KB static, <= 56 VGPRs, no scratch; correct for any
//   coordinates.
//
// alt_corr_bwd_scatter_kernel: the `tiled` dF2 path. Workgroup = 4 x 4
//   target pixels x one level x one 64-channel slice, 256 threads. A box
//   of (K+1+4)^2 level cells (14 x 14 at R = 4, 12 x 12 at R = 3) is
//   anchored at the tile's minimum window origin. The 16 pixels' patch
//   gradients are first written to LDS in BOX coordinates, dpb[cell][pixel]
//   (12.3 KB; zero where a cell is outside a pixel's patch or the map).
//   Then lane = channel and box row `by` belongs to wave by % 4: a wave
//   walks its cells, sums the 16 pixels' terms dpb[cell][p] * f1[p][ch] in
//   a register (four 16-byte LDS broadcasts + 16 FMAs per cell, f1 in 16
//   VGPRs) and issues ONE 256-byte atomic per touched in-map cell -- the
//   box itself never exists in memory, no LDS adds, no races. In-map
//   positions outside the box ("spill") take the direct kernel's atomic.
//   LDS 18.3 KB static, 47 VGPRs -> 8 workgroups = 32 waves per CU. Atomic
//   bytes per tile-level fall from 16 (K+1)^2 D 4 to <= box^2 D 4 (8.2x at
//   R = 4) when the tile's windows overlap, and degrade to the direct count
//   when not.
//
// alt_corr_bwd_finalize_kernel: the pooling-chain gather above, 16 bytes
//   per thread.
//
// Safety: coordinates are clamped in float before the int conversion
// (acb_axis); a window that misses the map is skipped before any address
// is formed; every position is bounds-checked. The pad tail of an NHWC
// cotangent is never read. No host sync, no allocation.

#include "alt_corr_bwd_maps.h"
#include "common.h"

struct AcbLevels {
  const __bf16* p[4];  // pooled f2, (B, Hl, Wl, D) channels-last bf16
  float* acc[4];       // fp32 level-gradient accumulators, same shape
  int H[4];
  int W[4];
};

__device__ __forceinline__ float acb_load_g(const void* g, long off, int bf) {
  return bf ? (float)((const __bf16*)g)[off] : ((const float*)g)[off];
}

__device__ __forceinline__ float acb_uniform(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

__device__ __forceinline__ void acb_atomic_add(float* p, float v) {
  // result unused: a no-return global_atomic_add_f32
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// transposed separable blend of one patch position; gs = the level's K*K
// cotangents, wx/wy = {w0, w1}
__device__ __forceinline__ float acb_dpatch(const float* gs, int j, int a,
                                            int K, const float wx[2],
                                            const float wy[2]) {
  int tap[4];
  const int mask = acb_taps(j, a, K, tap);
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (mask >> k & 1) s += gs[tap[k]] * wy[k >> 1] * wx[k & 1];
  return s;
}

using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;  // 2 VGPRs

// df1 of one (pixel, level) when no atomics ride along: lane owns channel
// quads (lane + 64 n) * 4, one 8-byte read per lane covers 256 channels of
// an F2 row. The x loop is branch-free and fully unrolled so a row's KP
// reads are in flight together: an out-of-map column reads the clamped
// (in-map) cell of the same row and multiplies it by its dpatch, which is
// stored as zero.
template <int KP, int NV>
__device__ __forceinline__ void acb_df1_rows(const __bf16* __restrict__ f2b,
                                             const float* dps_l, int x0,
                                             int y0, int Wl, int Hl, int D,
                                             int lane, float (&acc)[NV][4]) {
  for (int j = 0; j < KP; ++j) {
    const int yy = y0 + j;
    if (yy < 0 || yy >= Hl) continue;
    const __bf16* rowb = f2b + (long)yy * Wl * D;
#pragma unroll
    for (int a = 0; a < KP; ++a) {
      const int xx = min(max(x0 + a, 0), Wl - 1);
      const float dp = dps_l[j * KP + a];
#pragma unroll
      for (int n = 0; n < NV; ++n) {
        const int ch = (lane + 64 * n) * 4;
        if (ch < D) {
          const bf16x4 v =
              *reinterpret_cast<const bf16x4*>(rowb + (long)xx * D + ch);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[n][e] += dp * (float)v[e];
        }
      }
    }
  }
}

template <int NC, bool ATOMICS>
__global__ __launch_bounds__(256) void alt_corr_bwd_direct_kernel(
    const __bf16* __restrict__ f1,     // (B*P, D) bf16 rows
    AcbLevels lv,
    const float* __restrict__ coords,  // (B, 2, H, W)
    const void* __restrict__ grad,     // forward-output layout
    float* __restrict__ df1,           // (B*P, D) fp32 or null
    int P, int D, int L, int R, int cl, int ldc, int g_bf16, int need_f1,
    int need_f2, float scale) {
  const int K = 2 * R + 1, KP = K + 1, K2 = K * K, NPOS = KP * KP;
  __shared__ float gs[4][ACB_MAX_K2 + 3];
  __shared__ float dps[4][ACB_MAX_NPOS];
  __shared__ __attribute__((aligned(16))) float red[4][512];

  const int lane = threadIdx.x & 63;
  const int l = threadIdx.x >> 6;      // wave = level, l < L by launch
  const int pix = blockIdx.x;
  const int b = pix / P, i = pix - b * P;
  const int Hl = lv.H[l], Wl = lv.W[l];

  const float inv = 1.0f / (float)(1 << l);
  int x0, y0;
  float wx[2], wy[2];
  acb_axis(coords[((long)b * 2 + 0) * P + i] * inv, Wl, R, &x0, &wx[0], &wx[1]);
  acb_axis(coords[((long)b * 2 + 1) * P + i] * inv, Hl, R, &y0, &wy[0], &wy[1]);
  // wave-uniform: a window that misses the map contributes nothing
  const bool hits = acb_axis_hits(x0, K, Wl) & acb_axis_hits(y0, K, Hl);

  if (hits) {
    for (int o = lane; o < K2; o += 64)
      gs[l][o] = acb_load_g(
          grad, acb_grad_off(b, i, l * K2 + o, P, L * K2, cl, ldc), g_bf16);
  }
  __syncthreads();
  if (hits) {
    for (int pos = lane; pos < NPOS; pos += 64) {
      const int j = pos / KP, a = pos - j * KP;
      float dp = 0.0f;
      if (acb_in_map(x0 + a, y0 + j, Wl, Hl))
        dp = acb_dpatch(gs[l], j, a, K, wx, wy) * scale;
      dps[l][pos] = dp;
    }
  }
  __syncthreads();

  if constexpr (!ATOMICS) {
    // df1 only (the `tiled` path; need_f1 holds by launch)
    constexpr int NV = (NC + 3) / 4;
    float acc[NV][4];
#pragma unroll
    for (int n = 0; n < NV; ++n)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[n][e] = 0.0f;
    if (hits) {
      const __bf16* f2b = lv.p[l] + (long)b * Hl * Wl * D;
      if (R == 4)
        acb_df1_rows<10, NV>(f2b, dps[l], x0, y0, Wl, Hl, D, lane, acc);
      else
        acb_df1_rows<8, NV>(f2b, dps[l], x0, y0, Wl, Hl, D, lane, acc);
    }
#pragma unroll
    for (int n = 0; n < NV; ++n) {
      const int ch = (lane + 64 * n) * 4;
      if (ch < 512)
        *reinterpret_cast<f32x4*>(&red[l][ch]) =
            f32x4{acc[n][0], acc[n][1], acc[n][2], acc[n][3]};
    }
  } else {
    float acc[NC];
#pragma unroll
    for (int n = 0; n < NC; ++n) acc[n] = 0.0f;

    if (hits) {
      float q[NC];
#pragma unroll
      for (int n = 0; n < NC; ++n) {
        const int ch = lane + 64 * n;
        q[n] = ch < D ? (float)f1[(long)pix * D + ch] : 0.0f;
      }
      const __bf16* f2b = lv.p[l] + (long)b * Hl * Wl * D;
      float* accb = lv.acc[l] + (long)b * Hl * Wl * D;
      for (int j = 0; j < KP; ++j) {
        const int yy = y0 + j;
        if (yy < 0 || yy >= Hl) continue;
        for (int a = 0; a < KP; ++a) {
          const int xx = x0 + a;
          if (xx < 0 || xx >= Wl) continue;
          const float dp = acb_uniform(dps[l][j * KP + a]);
          if (dp == 0.0f) continue;
          const long row = ((long)yy * Wl + xx) * D;
#pragma unroll
          for (int n = 0; n < NC; ++n) {
            const int ch = lane + 64 * n;
            if (ch < D) {
              if (need_f1) acc[n] += dp * (float)f2b[row + ch];
              if (need_f2) acb_atomic_add(accb + row + ch, dp * q[n]);
            }
          }
        }
      }
    }
    if (!need_f1) return;  // block-uniform
#pragma unroll
    for (int n = 0; n < NC; ++n) red[l][lane + 64 * n] = acc[n];
  }
  __syncthreads();
  for (int ch = threadIdx.x; ch < D; ch += blockDim.x) {
    float s = 0.0f;
    for (int w = 0; w < L; ++w) s += red[w][ch];
    df1[(long)pix * D + ch] = s;
  }
}

__global__ __launch_bounds__(256) void alt_corr_bwd_scatter_kernel(
    const __bf16* __restrict__ f1, AcbLevels lv,
    const float* __restrict__ coords, const void* __restrict__ grad,
    int H, int W, int D, int L, int R, int cl, int ldc, int g_bf16,
    float scale) {
  const int K = 2 * R + 1, KP = K + 1, K2 = K * K;
  const int box = acb_box_side(R);
  const int P = H * W;

  // dpb[slot][p]: patch gradient of tile pixel p at box cell `slot`
  // (zero where the cell is outside p's patch or outside the map)
  __shared__ __attribute__((aligned(16))) float
      dpb[ACB_MAX_BOX * ACB_MAX_BOX][ACB_NPIX];
  __shared__ float gs[ACB_NPIX][ACB_MAX_K2];
  __shared__ float wts[ACB_NPIX][4];
  __shared__ int org[ACB_NPIX][2];
  __shared__ int hit_s[ACB_NPIX];
  __shared__ int pix_s[ACB_NPIX];
  __shared__ int spill_s[ACB_NPIX];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int l = blockIdx.y;
  const int ch = blockIdx.z * ACB_SLICE + lane;
  const bool chv = ch < D;
  const int Hl = lv.H[l], Wl = lv.W[l];
  int b, ty, tx;
  acb_tile_decode(blockIdx.x, H, W, &b, &ty, &tx);

  if (tid < ACB_NPIX) {
    const int py = ty + tid / ACB_TILE, px = tx + tid % ACB_TILE;
    int hit = 0, x0 = 0, y0 = 0, i = 0;
    float w[4] = {0.f, 0.f, 0.f, 0.f};
    if (py < H && px < W) {
      i = py * W + px;
      const float inv = 1.0f / (float)(1 << l);
      acb_axis(coords[((long)b * 2 + 0) * P + i] * inv, Wl, R, &x0, &w[0], &w[1]);
      acb_axis(coords[((long)b * 2 + 1) * P + i] * inv, Hl, R, &y0, &w[2], &w[3]);
      hit = acb_axis_hits(x0, K, Wl) & acb_axis_hits(y0, K, Hl);
    }
    org[tid][0] = x0;
    org[tid][1] = y0;
    hit_s[tid] = hit;
    pix_s[tid] = i;
#pragma unroll
    for (int k = 0; k < 4; ++k) wts[tid][k] = w[k];
  }
  __syncthreads();

  int ax = ACB_NO_ANCHOR, ay = ACB_NO_ANCHOR;
  for (int p = 0; p < ACB_NPIX; ++p) {
    if (hit_s[p]) {
      ax = acb_anchor_fold(ax, org[p][0]);
      ay = acb_anchor_fold(ay, org[p][1]);
    }
  }
  if (ax == ACB_NO_ANCHOR) return;  // block-uniform: no window meets the map

  for (int idx = tid; idx < ACB_NPIX * K2; idx += 256) {
    const int p = idx / K2, o = idx - p * K2;
    if (hit_s[p])
      gs[p][o] = acb_load_g(
          grad, acb_grad_off(b, pix_s[p], l * K2 + o, P, L * K2, cl, ldc),
          g_bf16);
  }
  __syncthreads();
  // box-relative patch gradients, one (cell, pixel) per thread and step
  for (int idx = tid; idx < box * box * ACB_NPIX; idx += 256) {
    const int p = idx & (ACB_NPIX - 1), slot = idx / ACB_NPIX;
    const int by = slot / box, bx = slot - by * box;
    const int xx = ax + bx, yy = ay + by;
    const int a = xx - org[p][0], j = yy - org[p][1];
    float dp = 0.0f;
    if (hit_s[p] && (a >= 0) & (a < KP) & (j >= 0) & (j < KP) &&
        acb_in_map(xx, yy, Wl, Hl)) {
      const float wx[2] = {wts[p][0], wts[p][1]};
      const float wy[2] = {wts[p][2], wts[p][3]};
      dp = acb_dpatch(gs[p], j, a, K, wx, wy) * scale;
    }
    dpb[slot][p] = dp;
  }
  if (tid < ACB_NPIX) {
    // does the in-map part of this pixel's window leave the box?
    spill_s[tid] = hit_s[tid] &&
                   (acb_axis_spills(org[tid][0], K, Wl, ax, box) |
                    acb_axis_spills(org[tid][1], K, Hl, ay, box));
  }
  __syncthreads();

  float* accb = lv.acc[l] + (long)b * Hl * Wl * D;
  float q[ACB_NPIX];
#pragma unroll
  for (int p = 0; p < ACB_NPIX; ++p)
    q[p] = (chv && hit_s[p])
               ? (float)f1[((long)b * P + pix_s[p]) * D + ch] : 0.0f;

  // box cells: wave = rows by % 4, lane = channel; the 16 pixels' terms
  // are summed in a register and each touched in-map cell gets ONE
  // 256-byte atomic
  for (int by = wave; by < box; by += ACB_WAVES) {
    const int yy = ay + by;
    if (yy >= Hl) break;
    for (int bx = 0; bx < box; ++bx) {
      const int xx = ax + bx;
      if (xx >= Wl) break;
      const f32x4* dv = reinterpret_cast<const f32x4*>(dpb[by * box + bx]);
      float s = 0.0f;
      bool any = false;
#pragma unroll
      for (int v = 0; v < ACB_NPIX / 4; ++v) {
        const f32x4 d = dv[v];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s += d[e] * q[v * 4 + e];
          any |= d[e] != 0.0f;
        }
      }
      if (any && chv) acb_atomic_add(accb + ((long)yy * Wl + xx) * D + ch, s);
    }
  }

  // spill: in-map positions outside the box, straight to the accumulator
  for (int p = 0; p < ACB_NPIX; ++p) {
    if (!spill_s[p]) continue;  // block-uniform
    const float qp =
        chv ? (float)f1[((long)b * P + pix_s[p]) * D + ch] : 0.0f;
    const int x0 = org[p][0], y0 = org[p][1];
    const float wx[2] = {wts[p][0], wts[p][1]};
    const float wy[2] = {wts[p][2], wts[p][3]};
    for (int j = 0; j < KP; ++j) {
      const int yy = y0 + j;
      if (yy < 0 || yy >= Hl) continue;
      if (acb_row_owner(yy, ay) != wave) continue;
      for (int a = 0; a < KP; ++a) {
        const int xx = x0 + a;
        if (xx < 0 || xx >= Wl) continue;
        if (acb_box_slot(xx, yy, ax, ay, box) >= 0) continue;
        const float dp = acb_uniform(acb_dpatch(gs[p], j, a, K, wx, wy) * scale);
        if (dp == 0.0f) continue;
        if (chv) acb_atomic_add(accb + ((long)yy * Wl + xx) * D + ch, dp * qp);
      }
    }
  }
}

__global__ __launch_bounds__(256) void alt_corr_bwd_finalize_kernel(
    AcbLevels lv, float* __restrict__ df2,  // (B, H, W, D) fp32
    int B, int H, int W, int D, int L) {
  const int D4 = D >> 2;
  const long total = (long)B * H * W * D4;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c4 = (int)(idx % D4);
  long r = idx / D4;
  const int x = (int)(r % W);
  r /= W;
  const int y = (int)(r % H);
  const int b = (int)(r / H);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  float wgt = 1.0f;
  for (int l = 0; l < L; ++l) {
    const int Hl = lv.H[l], Wl = lv.W[l];
    if (acb_fin_member(y, x, l, Hl, Wl)) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(
          lv.acc[l] + (((long)b * Hl + (y >> l)) * Wl + (x >> l)) * D + c4 * 4);
      s += v * wgt;
    }
    wgt *= 0.25f;
  }
  *reinterpret_cast<f32x4*>(df2 + idx * 4) = s;
}

template <int NC>
static void acb_direct_launch(bool atomics, const __bf16* f1,
                              const AcbLevels& lv, const float* coords,
                              const void* grad, float* df1, int BP, int P,
                              int D, int L, int R, int cl, int ldc,
                              int g_bf16, int need_f1, int need_f2,
                              hipStream_t stream) {
  const float scale = 1.0f / sqrtf((float)D);
  if (atomics)
    hipLaunchKernelGGL((alt_corr_bwd_direct_kernel<NC, true>), dim3(BP),
                       dim3(64 * L), 0, stream, f1, lv, coords, grad, df1, P,
                       D, L, R, cl, ldc, g_bf16, need_f1, need_f2, scale);
  else
    hipLaunchKernelGGL((alt_corr_bwd_direct_kernel<NC, false>), dim3(BP),
                       dim3(64 * L), 0, stream, f1, lv, coords, grad, df1, P,
                       D, L, R, cl, ldc, g_bf16, need_f1, 0, scale);
}

bool flowhip_alt_corr_supported(int D, int radius, int L);

// algo: 0 = direct, 1 = tiled. `accs` are zero-initialised fp32 level
// accumulators (only touched when need_f2); df1 / df2 may be null when not
// needed.
bool flowhip_alt_corr_lookup_bwd_launch(
    const void* f1, const void* const* levels, float* const* accs,
    const int* Hs, const int* Ws, const float* coords, const void* grad,
    float* df1, float* df2, int B, int H, int W, int D, int L, int radius,
    int cl, int ldc, int g_bf16, int need_f1, int need_f2, int algo,
    hipStream_t stream) {
  if (!flowhip_alt_corr_supported(D, radius, L)) return false;
  if (algo != 0 && algo != 1) return false;
  if (!need_f1 && !need_f2) return true;
  AcbLevels lv{};
  for (int l = 0; l < L; ++l) {
    lv.p[l] = (const __bf16*)levels[l];
    lv.acc[l] = accs[l];
    lv.H[l] = Hs[l];
    lv.W[l] = Ws[l];
  }
  const int P = H * W, BP = B * P;
  const __bf16* a = (const __bf16*)f1;
  const bool tiled = algo == 1;
  const bool atomics = !tiled && need_f2;
  if (need_f1 || atomics) {
#define ACB_CASE(n)                                                          \
  case n:                                                                    \
    acb_direct_launch<n>(atomics, a, lv, coords, grad, df1, BP, P, D, L,     \
                         radius, cl, ldc, g_bf16, need_f1, need_f2, stream); \
    break;
    switch (fh_cdiv(D, 64)) {
      ACB_CASE(1) ACB_CASE(2) ACB_CASE(3) ACB_CASE(4)
      ACB_CASE(5) ACB_CASE(6) ACB_CASE(7) ACB_CASE(8)
      default: return false;
    }
#undef ACB_CASE
  }
  if (need_f2) {
    if (tiled) {
      const int tiles = B * fh_cdiv(H, ACB_TILE) * fh_cdiv(W, ACB_TILE);
      hipLaunchKernelGGL(alt_corr_bwd_scatter_kernel,
                         dim3(tiles, L, fh_cdiv(D, ACB_SLICE)), dim3(256), 0,
                         stream, a, lv, coords, grad, H, W, D, L, radius, cl,
                         ldc, g_bf16, 1.0f / sqrtf((float)D));
    }
    const long total = (long)BP * (D / 4);
    hipLaunchKernelGGL(alt_corr_bwd_finalize_kernel,
                       dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       stream, lv, df2, B, H, W, D, L);
  }
  return true;
}
