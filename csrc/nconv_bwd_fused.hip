// Fused normalized-convolution backward: one pass over the planes of a
// layer produces ddata, dconf and the per-workgroup partials of dweight /
// dbias; a small reduce kernel finishes them. Replaces the prep, bwd-data,
// wrw(+reduce) and plane-dot kernels of nconv.hip and the torch glue
// around them (math contract: header of flowhip/ops/functional_nconv.py).
//
//   de     = cout * s[co] + eps,  s[co] = sum(w[co])   (denom from cout)
//   dnomin = gout / de
//   ddenom = -dnomin * (out - bias[co])  [+ gcout / s[co]]
//   g  = convT(dnomin, w[.,ci]);  gd = convT(ddenom, w[.,ci])
//   ddata = conf * g ;  dconf = data * g + gd
//   dw[co,ci,ky,kx] = sum_q dc[ci,q] * dnomin[co,q-d] + c[ci,q] * ddenom[co,q-d]
//                     - sum(cout * gcout)[co] / s[co],   d = (ky-K/2, kx-K/2)
//   dbias[co] = sum gout[co]
//
// A 256-thread workgroup walks a strip of 64x16 tiles down one tile column.
// Per tile it computes (dnomin, ddenom) for the tile plus a K/2 halo while
// staging them into LDS (zeros outside the image; they never reach HBM).
// Each thread owns 4 adjacent pixels: data/conf come from plain float4
// loads at those pixels, and one (K+3)-wide LDS row read per (co, ky)
// feeds both the transposed-conv gather and the input-centred weight
// gradient products. The weight-gradient accumulators live in registers
// for the whole strip (every index is a compile-time constant) and are
// reduced across lanes once per workgroup. Requires W % 4 == 0.

#include <type_traits>

#include "common.h"
#include "nconv.h"

#define NBF_THREADS 256
#define NBF_TW NCONV_TW
#define NBF_TH NCONV_TH

// LDS row stride: halo row rounded up to whole float4s, so the row reads
// are 16-B aligned.
template <int K>
constexpr int nbf_lw() {
  return (NBF_TW + K - 1 + 3) & ~3;
}

// Output channels whose accumulators are register-resident together
// (<= 100 accumulators). With one group they persist over the strip;
// otherwise each group is reduced into LDS per tile.
template <int K, int CI, int CO>
constexpr int nbf_cog() {
  int g = 100 / (CI * K * K);
  if (g < 1) g = 1;
  if (g > CO) g = CO;
  while (CO % g) --g;
  return g;
}

// Waves per SIMD the register budget is sized for: 2 where all of a
// layer's accumulators are resident (every flagship layer); the grouped
// instances carry 4 or 8 input channels of data / conf / gradients beside
// a full group and get the whole register file.
template <int K, int CI, int CO>
constexpr int nbf_min_waves() {
  return CO / nbf_cog<K, CI, CO>() > 1 ? 1 : 2;
}

// Stage (dnomin, ddenom) of the tile at (x0, y0) plus halo. Aligned float4
// chunks cover [x0-4, x0+TW+4); with W % 4 == 0 a chunk is wholly inside
// or wholly outside the image, so no access is clamped or split. Adds the
// tile interior's gout and cout*gcout into (sg, sdot).
template <int K, int CO>
__device__ inline void nbf_stage(const float* __restrict__ gout,
                                 const float* __restrict__ gcout,
                                 const float* __restrict__ out,
                                 const float* __restrict__ cout,
                                 const float (&s)[CO], const float (&b)[CO],
                                 float eps, float* __restrict__ lds_gn,
                                 float* __restrict__ lds_gd, int n, int x0,
                                 int y0, int H, int W, float (&sg)[CO],
                                 float (&sdot)[CO]) {
  constexpr int R = K / 2;
  constexpr int LW = nbf_lw<K>();
  constexpr int LH = NBF_TH + K - 1;
  constexpr int CHUNKS = (NBF_TW + 8) / 4;  // 18 aligned float4 per row
  const long plane = (long)H * W;
  for (int u = threadIdx.x; u < LH * CHUNKS; u += NBF_THREADS) {
    const int row = u / CHUNKS, k = u - row * CHUNKS;
    const int gy = y0 - R + row;
    const int gx = x0 - 4 + k * 4;
    const bool in = (gy >= 0 && gy < H && gx >= 0 && gx < W);
    const bool interior = in && row >= R && row < R + NBF_TH && k >= 1 &&
                          k <= NBF_TW / 4;
    const int lc0 = gx - (x0 - R);
#pragma unroll
    for (int co = 0; co < CO; ++co) {
      float4 dn = {0.f, 0.f, 0.f, 0.f}, dd = {0.f, 0.f, 0.f, 0.f};
      if (in) {
        const long p = ((long)n * CO + co) * plane + (long)gy * W + gx;
        const float4 c4 = *(const float4*)(cout + p);
        float4 go4 = {0.f, 0.f, 0.f, 0.f}, o4 = {0.f, 0.f, 0.f, 0.f};
        float4 gc4 = {0.f, 0.f, 0.f, 0.f};
        if (gout != nullptr) {
          go4 = *(const float4*)(gout + p);
          o4 = *(const float4*)(out + p);
        }
        if (gcout != nullptr) gc4 = *(const float4*)(gcout + p);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float go = (&go4.x)[e];
          const float de = (&c4.x)[e] * s[co] + eps;
          const float ratio = (&o4.x)[e] - b[co];
          // ddenom from the ROUNDED dnomin: dc*dnomin and c*ddenom cancel
          // in the weight gradient (exactly where a window holds a single
          // sample, out == data), and only then does dnomin's rounding
          // scale the pair instead of breaking the cancellation. With
          // both rounded on their own from gout/de, that term alone was
          // 2.6e-5 of dweight error in the zero-inject case, against
          // 1e-5 for exact arithmetic on the same saved out / cout.
          const float dne = go / de;
          float d = -dne * ratio;
          if (gcout != nullptr) d += (&gc4.x)[e] / s[co];
          (&dn.x)[e] = dne;
          (&dd.x)[e] = d;
        }
        if (interior) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            sg[co] += (&go4.x)[e];
            sdot[co] += (&c4.x)[e] * (&gc4.x)[e];
          }
        }
      }
      float* ln = lds_gn + (co * LH + row) * LW;
      float* ld = lds_gd + (co * LH + row) * LW;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int lcol = lc0 + e;
        if (lcol >= 0 && lcol < NBF_TW + K - 1) {
          ln[lcol] = (&dn.x)[e];
          ld[lcol] = (&dd.x)[e];
        }
      }
    }
  }
}

// acc += a * b as one v_fmac_f32. Written as an instruction because the
// compiler's SLP pass otherwise pairs the unrolled multiply-adds into
// packed fp32 ops whose operand shuffles more than double the register
// count (174 VGPRs at <5,1,1> against 76) and push <5,2,2> into scratch.
__device__ __forceinline__ void nbf_fmac(float& acc, float a, float b) {
  asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(a), "v"(b));
}

// Wave-shuffle sum of each of the N values; lane 0 stores (or adds) them
// into dst. Must be called by whole waves. T is the type the 64 lanes are
// summed in: fp64 for up to 50 accumulators and for the 2*Co whole-image
// sums behind dbias and the cout*gcout term (few values per thread, so the
// lane tree is their error), fp32 for the 72- and 100-accumulator layers,
// where fp64 shuffles cost 10 us per call (twice the LDS-crossbar traffic).
// The sums over waves and workgroups after it are always fp64.
template <int N, bool ADD, typename T = float, typename S = float>
__device__ inline void nbf_wave_reduce(const S (&v)[N],
                                       double* __restrict__ dst, int lane) {
  constexpr int G = 8;  // values in flight: hides the shuffle latency
#pragma unroll
  for (int i0 = 0; i0 < N; i0 += G) {
    T x[G];
#pragma unroll
    for (int j = 0; j < G; ++j) x[j] = i0 + j < N ? (T)v[i0 + j] : (T)0;
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1)
#pragma unroll
      for (int j = 0; j < G; ++j)
        if (i0 + j < N) x[j] += __shfl_down(x[j], sh, 64);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < G; ++j)
        if (i0 + j < N) {
          if (ADD) dst[i0 + j] += (double)x[j];
          else dst[i0 + j] = (double)x[j];
        }
    }
    // bounds the registers the unrolled shuffles hold
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Grid: ntx * nstrips * N workgroups; workgroup = tile column tx, tile rows
// [sidx*strip, min((sidx+1)*strip, nty)) of sample n.
// partials row: [Co*Ci*K*K dweight sums | Co sums of cout*gcout | Co sums
// of gout].
template <int K, int CI, int CO>
__global__ __launch_bounds__(NBF_THREADS, (nbf_min_waves<K, CI, CO>()))
void nconv_bwd_fused_kernel(
    const float* __restrict__ gout, const float* __restrict__ gcout,
    const float* __restrict__ out, const float* __restrict__ cout,
    const float* __restrict__ data, const float* __restrict__ conf,
    const float* __restrict__ weight, const float* __restrict__ bias,
    float* __restrict__ ddata, float* __restrict__ dconf,
    float* __restrict__ partials, int H, int W, int ntx, int nty, int strip,
    int nstrips, float eps) {
  constexpr int LW = nbf_lw<K>();
  constexpr int LH = NBF_TH + K - 1;
  constexpr int NW = CI * K * K;   // weights per co
  constexpr int NWT = CO * NW;
  constexpr int NCOL = NWT + 2 * CO;
  constexpr int COG = nbf_cog<K, CI, CO>();
  constexpr int NG = CO / COG;
  __shared__ __attribute__((aligned(16))) float lds_gn[CO * LH * LW];
  __shared__ __attribute__((aligned(16))) float lds_gd[CO * LH * LW];
  __shared__ double red[4 * NCOL];

  int t = blockIdx.x;
  const int tx = t % ntx; t /= ntx;
  const int sidx = t % nstrips;
  const int n = t / nstrips;
  const int x0 = tx * NBF_TW;
  const int ty_end = min((sidx + 1) * strip, nty);

  // s = sum(w) per out channel, summed in the forward kernel's order
  float s[CO], b[CO];
#pragma unroll
  for (int co = 0; co < CO; ++co) {
    float a = 0.f;
    for (int i = 0; i < NW; ++i) a += weight[co * NW + i];
    s[co] = a;
    b[co] = bias != nullptr ? bias[co] : 0.f;
  }

  const long plane = (long)H * W;
  const int lxb = (threadIdx.x & 15) * 4;   // tile-local x of pixel 0
  const int row = threadIdx.x >> 4;         // 0..15
  const int x = x0 + lxb;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;

  if (NG > 1)  // per-tile group sums accumulate here; first use is after
               // the first tile's barrier
    for (int i = threadIdx.x; i < 4 * NCOL; i += NBF_THREADS) red[i] = 0.0;

  // the 1x1 layers (at most 8 accumulators) stream memory and have the
  // VALU idle: they accumulate in fp64 outright
  constexpr bool F64ACC = COG * NW <= 8;
  using AccT = typename std::conditional<F64ACC, double, float>::type;
  AccT acc[COG * NW];
#pragma unroll
  for (int i = 0; i < COG * NW; ++i) acc[i] = 0.f;
  float sdot[CO], sg[CO];
#pragma unroll
  for (int co = 0; co < CO; ++co) { sdot[co] = 0.f; sg[co] = 0.f; }

#pragma unroll 1
  for (int ty = sidx * strip; ty < ty_end; ++ty) {
    const int y0 = ty * NBF_TH;
    nbf_stage<K, CO>(gout, gcout, out, cout, s, b, eps, lds_gn, lds_gd, n, x0,
                     y0, H, W, sg, sdot);
    __syncthreads();

    // W % 4 == 0: the thread's 4 pixels are all inside or all outside.
    // Outside threads skip the compute and the stores.
    const int y = y0 + row;
    const bool active = (x < W && y < H);
    float c[CI][4], d[CI][4], dc[CI][4];
#pragma unroll
    for (int ci = 0; ci < CI; ++ci) {
      float4 c4 = {0.f, 0.f, 0.f, 0.f}, d4 = {0.f, 0.f, 0.f, 0.f};
      if (active) {
        const long p = ((long)n * CI + ci) * plane + (long)y * W + x;
        c4 = *(const float4*)(conf + p);
        d4 = *(const float4*)(data + p);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        c[ci][e] = (&c4.x)[e];
        d[ci][e] = (&d4.x)[e];
        dc[ci][e] = (&d4.x)[e] * (&c4.x)[e];
      }
    }
    float g[CI][4], gd[CI][4];
#pragma unroll
    for (int ci = 0; ci < CI; ++ci)
#pragma unroll
      for (int e = 0; e < 4; ++e) { g[ci][e] = 0.f; gd[ci][e] = 0.f; }

#pragma unroll 1
    for (int grp = 0; grp < NG; ++grp) {
      if (NG > 1) {
#pragma unroll
        for (int i = 0; i < COG * NW; ++i) acc[i] = 0.f;
      }
      // whole compute under `active` (the wave reductions are not): left
      // unconditional, g/gd are sunk into the store branch below and keep
      // every row buffer live
      if (active) {
#pragma unroll
      for (int cl = 0; cl < COG; ++cl) {
        const int co = grp * COG + cl;
        const float* lgn = lds_gn + co * LH * LW;
        const float* lgd = lds_gd + co * LH * LW;
        const float* wco = weight + co * NW;  // uniform -> scalar loads
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
          // LDS(r, c) = dout(y0 - K/2 + r, x0 - K/2 + c), so dout(q - d) of
          // pixel e sits at row + K-1-ky, column lxb + e + K-1-kx
          float nbuf[(K + 3 + 3) & ~3], dbuf[(K + 3 + 3) & ~3];
          const float* rn = lgn + (row + K - 1 - ky) * LW + lxb;
          const float* rd = lgd + (row + K - 1 - ky) * LW + lxb;
#pragma unroll
          for (int q = 0; q < (K + 3) / 4; ++q) {
            const float4 vn = *(const float4*)(rn + 4 * q);
            const float4 vd = *(const float4*)(rd + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              nbuf[4 * q + e] = (&vn.x)[e];
              dbuf[4 * q + e] = (&vd.x)[e];
            }
          }
          if constexpr ((K + 3) % 4 == 2) {  // K == 3: taps 4, 5
            constexpr int o = (K + 3) / 4 * 4;
            const float2 vn = *(const float2*)(rn + o);
            const float2 vd = *(const float2*)(rd + o);
            nbuf[o] = vn.x; nbuf[o + 1] = vn.y;
            dbuf[o] = vd.x; dbuf[o + 1] = vd.y;
          }
#pragma unroll
          for (int ci = 0; ci < CI; ++ci) {
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
              const float w = wco[(ci * K + ky) * K + kx];
              AccT v = acc[((cl * CI + ci) * K + ky) * K + kx];
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float vn = nbuf[K - 1 - kx + e];
                const float vd = dbuf[K - 1 - kx + e];
                nbf_fmac(g[ci][e], w, vn);
                nbf_fmac(gd[ci][e], w, vd);
                if constexpr (F64ACC) {
                  v = __builtin_fma((double)dc[ci][e], (double)vn, v);
                  v = __builtin_fma((double)c[ci][e], (double)vd, v);
                } else {
                  nbf_fmac(v, dc[ci][e], vn);
                  nbf_fmac(v, c[ci][e], vd);
                }
              }
              acc[((cl * CI + ci) * K + ky) * K + kx] = v;
            }
          }
          // keep one row group's LDS reads in flight: without the fence
          // the scheduler hoists every row of the unrolled body and the
          // kernel runs out of registers
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      }
      if (NG > 1)
        nbf_wave_reduce<COG * NW, true, float, AccT>(
            acc, red + wave * NCOL + grp * COG * NW, lane);
    }

    if (active) {
#pragma unroll
      for (int ci = 0; ci < CI; ++ci) {
        const long p = ((long)n * CI + ci) * plane + (long)y * W + x;
        float4 vd, vc;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          (&vd.x)[e] = c[ci][e] * g[ci][e];
          (&vc.x)[e] = d[ci][e] * g[ci][e] + gd[ci][e];
        }
        *(float4*)(ddata + p) = vd;
        *(float4*)(dconf + p) = vc;
      }
    }
    __syncthreads();  // tile fully read before the next stage overwrites it
  }

  // up to 50 accumulators the fp64 lane sums cost nothing measurable
  using LaneT = typename std::conditional<(COG * NW <= 50), double, float>::type;
  if (NG == 1)
    nbf_wave_reduce<COG * NW, false, LaneT, AccT>(acc, red + wave * NCOL,
                                                  lane);
  nbf_wave_reduce<CO, false, double>(sdot, red + wave * NCOL + NWT, lane);
  nbf_wave_reduce<CO, false, double>(sg, red + wave * NCOL + NWT + CO, lane);
  __syncthreads();
  for (int i = threadIdx.x; i < NCOL; i += NBF_THREADS)
    partials[(long)blockIdx.x * NCOL + i] =
        (float)((red[i] + red[NCOL + i]) +
                (red[2 * NCOL + i] + red[3 * NCOL + i]));
}

// Stage 2. Workgroup w < Co*NW: dweight[w] = sum_b partials[b, w]
// - (sum_b partials[b, NWT + co]) / s[co] (second term only with gcout);
// workgroup NWT + co (launched only with bias): dbias[co]. The few hundred
// partials are summed in fp64 (fixed order), so the result carries the
// rounding of the per-workgroup sums only.
__global__ __launch_bounds__(NBF_THREADS) void nconv_bwd_fused_reduce_kernel(
    const float* __restrict__ partials, const float* __restrict__ weight,
    float* __restrict__ dweight, float* __restrict__ dbias, int nblocks,
    int NW, int Co, int has_gcout) {
  const int NWT = Co * NW, NCOL = NWT + 2 * Co;
  const int w = blockIdx.x;
  const bool is_w = w < NWT;
  const int co = is_w ? w / NW : w - NWT;
  const int col = is_w ? w : NWT + Co + co;
  const bool dot = is_w && has_gcout;
  double a = 0.0, q = 0.0;
  for (int bI = threadIdx.x; bI < nblocks; bI += NBF_THREADS) {
    a += (double)partials[(long)bI * NCOL + col];
    if (dot) q += (double)partials[(long)bI * NCOL + NWT + co];
  }
  __shared__ double red[8];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) {
    a += __shfl_down(a, sh, 64);
    q += __shfl_down(q, sh, 64);
  }
  if (lane == 0) { red[wave] = a; red[4 + wave] = q; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = (red[0] + red[1]) + (red[2] + red[3]);
    if (!is_w) {
      dbias[co] = (float)v;
    } else {
      if (dot) {
        double s = 0.0;
        for (int i = 0; i < NW; ++i) s += (double)weight[co * NW + i];
        v -= ((red[4] + red[5]) + (red[6] + red[7])) / s;
      }
      dweight[w] = (float)v;
    }
  }
}

// ---------------------------------------------------------------------------
// Launcher. The envelope is the family's (flowhip_nconv_launchable, nconv.h);
// outside it the plan is 0 rows and nothing is launched.
// ---------------------------------------------------------------------------

bool flowhip_nconv_bwd_fused_launch(
    const float* gout, const float* gcout, const float* out,
    const float* cout, const float* data, const float* conf,
    const float* weight, const float* bias, float* ddata, float* dconf,
    float* partials, float* dweight, float* dbias, const NConvGeom& g,
    int strip, float eps, hipStream_t stream) {
  const int nblocks = flowhip_nconv_bwd_fused_plan(g, &strip);
  if (nblocks == 0) return false;
  const int ntx = fh_cdiv(g.W, NBF_TW), nty = fh_cdiv(g.H, NBF_TH);
  const int nstrips = fh_cdiv(nty, strip);
  dim3 grid(nblocks), block(NBF_THREADS);
#define NBF_CASE_LAUNCH(KK, CIV, COV)                                        \
  if (g.K == KK && g.Ci == CIV && g.Co == COV)                               \
    hipLaunchKernelGGL((nconv_bwd_fused_kernel<KK, CIV, COV>), grid, block,  \
                       0, stream, gout, gcout, out, cout, data, conf,        \
                       weight, bias, ddata, dconf, partials, g.H, g.W, ntx,  \
                       nty, strip, nstrips, eps);
  FLOWHIP_NCONV_TABLE(NBF_CASE_LAUNCH)
#undef NBF_CASE_LAUNCH
  const int NW = g.Ci * g.K * g.K;
  hipLaunchKernelGGL(nconv_bwd_fused_reduce_kernel,
                     dim3(g.Co * NW + (bias != nullptr ? g.Co : 0)),
                     dim3(NBF_THREADS), 0, stream, partials, weight, dweight,
                     dbias, nblocks, NW, g.Co, gcout != nullptr ? 1 : 0);
  return true;
}
