// On-demand correlation window lookup (RAFT's `--alternate_corr` mode): the
// same (2r+1)^2 x L taps that corr_lookup.hip gathers out of the all-pairs
// pyramid, computed straight from the two feature maps so nothing of size
// P^2 ever exists.
//
// Average pooling and bilinear sampling are linear, so the level-l
// correlation map of target pixel i is
//     corr_l[i](y, x) = <f1[:, i], avgpool_l(f2)[:, y, x]> / sqrt(D)
// with the floor-mode 2x2 pooling the volume pyramid uses. The op layer
// pools f2 once per pair (fp32, rounded to bf16 once per level); this
// kernel does the per-iteration part.
//
// Output contract == corr_lookup_fwd_kernel (see that file's header for the
// x-offset-MAJOR channel order and the separable-window identity):
//     out[b, l*K2 + a*K + c, i]  samples  (x + (a-R), y + (c-R))
// grid_sample(align_corners=True, zeros) semantics, NCHW or NHWC with the
// 8-aligned channel stride `ldc` and a zeroed pad tail.
//
// Parallelization: ONE WAVE owns one (target pixel, level); a 256-thread
// block is 4 consecutive pixels, blockIdx.y = level (BP/4 x L workgroups:
// 7040 at the 440x1024 flagship shape). Inside the wave, lane = (g, t) with
// g = lane/16, t = lane%16: the 16 lanes of a group split the D channels in
// 16-byte pieces (piece t, t+16, ...), and the 4 groups take 4 x-adjacent
// patch positions per pass, so one wave-instruction reads 4 consecutive
// channels-last f2 rows. f1[i] lives in registers as fp32. Each lane keeps
// one fp32 partial sum per pass; 16 passes are reduced over the 16 lanes of
// a group with a multi-value butterfly (15 shuffle-adds instead of 16 x 4),
// after which lane t holds the finished dot product of pass t. The (K+1)^2
// patch goes through LDS into the separable 2-tap blend, one output tap
// per lane, so the NHWC stores are unit-stride.
//
// Safety: every patch position is bounds-checked (out-of-map positions are
// never read and contribute zero), and the level coordinate is clamped in
// float to [-(R+2), extent+R+1] before the float->int conversion -- outside
// that band every tap is zero anyway, so +-1e6 or NaN coordinates give
// zeros and never form a wild address. No atomics, no host sync, no
// allocation: hipGraph-capturable.

#include "common.h"

#define AC_THREADS 256
#define AC_WAVES (AC_THREADS / 64)
#define AC_MAX_PATCH 100  // (2*4+2)^2

struct AcLevels {
  const __bf16* p[4];  // pooled f2, (B, Hl, Wl, D) channels-last bf16
  int H[4];
  int W[4];
};

// Reduce v[0..16) over the 16 lanes of a group: on return lane t's v[0]
// is the group sum of value t. Step `off` halves the live values: a lane
// keeps the half selected by its `off` bit and hands the other half over.
__device__ __forceinline__ float ac_reduce16(float (&v)[16], int t) {
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) {
    const bool hi = (t & off) != 0;
#pragma unroll
    for (int j = 0; j < off; ++j) {
      const float keep = hi ? v[j + off] : v[j];
      const float send = hi ? v[j] : v[j + off];
      v[j] = keep + __shfl_xor(send, off, 64);
    }
  }
  return v[0];
}

template <int R, int NC, typename out_t>
__global__ __launch_bounds__(AC_THREADS) void alt_corr_lookup_fwd_kernel(
    const __bf16* __restrict__ f1,     // (B*P, D) bf16 rows
    AcLevels lv,
    const float* __restrict__ coords,  // (B, 2, H, W)
    out_t* __restrict__ out,           // (B, L*K2, H, W) NCHW or NHWC
    int BP, int P, int D, int L, int cl, int ldc, float scale) {
  constexpr int K = 2 * R + 1;
  constexpr int K2 = K * K;
  constexpr int KP = K + 1;           // patch side
  constexpr int NPOS = KP * KP;       // 64 (R=3) or 100 (R=4)
  constexpr int NPASS = NPOS / 4;     // 16 or 25
  constexpr int NROUND = (NPASS + 15) / 16;
  static_assert(NPOS % 4 == 0 && NPOS <= AC_MAX_PATCH, "patch size");

  __shared__ float patch_s[AC_WAVES][AC_MAX_PATCH];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane >> 4, t = lane & 15;
  const int l = blockIdx.y;
  const int pix = blockIdx.x * AC_WAVES + wave;
  const bool live = pix < BP;          // wave-uniform; no early return
                                       // (the block meets at a barrier)
  const int Hl = lv.H[l], Wl = lv.W[l];
  float wx0 = 0.f, wx1 = 0.f, wy0 = 0.f, wy1 = 0.f;
  int b = 0, i = 0;

  if (live) {
    b = pix / P;
    i = pix - b * P;
    const float inv = 1.0f / (float)(1 << l);
    float cx = coords[((long)b * 2 + 0) * P + i] * inv;
    float cy = coords[((long)b * 2 + 1) * P + i] * inv;
    // clamp BEFORE float->int; fminf/fmaxf also replace NaN by the bound
    cx = fminf(fmaxf(cx, -(float)(R + 2)), (float)(Wl + R + 1));
    cy = fminf(fmaxf(cy, -(float)(R + 2)), (float)(Hl + R + 1));
    const float fx = floorf(cx), fy = floorf(cy);
    const int x0 = (int)fx - R;  // patch origin
    const int y0 = (int)fy - R;
    wx1 = cx - fx; wx0 = 1.0f - wx1;
    wy1 = cy - fy; wy0 = 1.0f - wy1;

    // f1 row -> fp32 registers, piece t + 16*n of 8 channels each
    float q[NC][8];
    bool pv[NC];
    const __bf16* f1row = f1 + (long)pix * D;
#pragma unroll
    for (int n = 0; n < NC; ++n) {
      const int ch = (t + 16 * n) * 8;
      pv[n] = ch < D;
      if (pv[n]) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(f1row + ch);
#pragma unroll
        for (int e = 0; e < 8; ++e) q[n][e] = (float)v[e];
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) q[n][e] = 0.0f;
      }
    }

    const __bf16* f2b = lv.p[l] + (long)b * Hl * Wl * D;
#pragma unroll
    for (int rd = 0; rd < NROUND; ++rd) {
      float acc[16];
#pragma unroll
      for (int pp = 0; pp < 16; ++pp) {
        acc[pp] = 0.0f;
        const int pass = rd * 16 + pp;
        if (pass < NPASS) {
          // 4 x-adjacent patch positions per pass, one per lane group
          const int pos = pass * 4 + g;
          const int j = pos / KP, a = pos - j * KP;
          const int xx = x0 + a, yy = y0 + j;
          if ((xx >= 0) & (xx < Wl) & (yy >= 0) & (yy < Hl)) {
            const __bf16* row = f2b + ((long)yy * Wl + xx) * D;
            float s = 0.0f;
#pragma unroll
            for (int n = 0; n < NC; ++n) {
              if (pv[n]) {
                const bf16x8 v = *reinterpret_cast<const bf16x8*>(
                    row + (t + 16 * n) * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) s += q[n][e] * (float)v[e];
              }
            }
            acc[pp] = s;
          }
        }
      }
      const float dot = ac_reduce16(acc, t);
      // lane (g, t) now owns pass rd*16 + t
      const int pass = rd * 16 + t;
      if (pass < NPASS) patch_s[wave][pass * 4 + g] = dot * scale;
    }
  }
  __syncthreads();
  if (!live) return;

  // separable blend: patch_s[j*KP + a] is the dot at (x0 + a, y0 + j)
  const float* ps = patch_s[wave];
  const long tap_stride = cl ? 1 : (long)P;
  out_t* outb = cl ? out + ((long)b * P + i) * ldc + (long)l * K2
                   : out + ((long)b * L * K2 + (long)l * K2) * P + i;
  for (int o = lane; o < K2; o += 64) {
    const int a = o / K, c = o - a * K;
    const float t0 = wy0 * ps[c * KP + a] + wy1 * ps[(c + 1) * KP + a];
    const float t1 = wy0 * ps[c * KP + a + 1] + wy1 * ps[(c + 1) * KP + a + 1];
    outb[(long)o * tap_stride] = (out_t)(wx0 * t0 + wx1 * t1);
  }
  if (cl && l == 0) {
    // zero the channel-pad tail once (ldc > L*K2, see corr_lookup.hip)
    out_t* rowb = out + ((long)b * P + i) * ldc;
    for (int c = L * K2 + lane; c < ldc; c += 64) rowb[c] = (out_t)0.0f;
  }
}

template <int R, int NC, typename out_t>
static void alt_fwd_launch(const __bf16* f1, const AcLevels& lv,
                           const float* coords, out_t* out, int BP, int P,
                           int D, int L, int cl, int ldc, hipStream_t stream) {
  dim3 grid(fh_cdiv(BP, AC_WAVES), L);
  hipLaunchKernelGGL((alt_corr_lookup_fwd_kernel<R, NC, out_t>), grid,
                     dim3(AC_THREADS), 0, stream, f1, lv, coords, out, BP, P,
                     D, L, cl, ldc, 1.0f / sqrtf((float)D));
}

template <int R, typename out_t>
static bool alt_fwd_nc(const __bf16* f1, const AcLevels& lv,
                       const float* coords, out_t* out, int BP, int P, int D,
                       int L, int cl, int ldc, hipStream_t stream) {
  switch (fh_cdiv(D, 128)) {
    case 1: alt_fwd_launch<R, 1>(f1, lv, coords, out, BP, P, D, L, cl, ldc, stream); return true;
    case 2: alt_fwd_launch<R, 2>(f1, lv, coords, out, BP, P, D, L, cl, ldc, stream); return true;
    case 3: alt_fwd_launch<R, 3>(f1, lv, coords, out, BP, P, D, L, cl, ldc, stream); return true;
    case 4: alt_fwd_launch<R, 4>(f1, lv, coords, out, BP, P, D, L, cl, ldc, stream); return true;
    default: return false;
  }
}

// D % 8 == 0, D <= 512, radius in {3, 4}, 1 <= L <= 4
bool flowhip_alt_corr_supported(int D, int radius, int L) {
  return D > 0 && D % 8 == 0 && D <= 512 && (radius == 3 || radius == 4) &&
         L >= 1 && L <= 4;
}

bool flowhip_alt_corr_lookup_fwd_launch(const void* f1,
                                        const void* const* levels,
                                        const int* Hs, const int* Ws,
                                        const float* coords, void* out,
                                        int BP, int P, int D, int L,
                                        int radius, int cl, int ldc,
                                        int out_bf16, hipStream_t stream) {
  if (!flowhip_alt_corr_supported(D, radius, L)) return false;
  AcLevels lv{};
  for (int l = 0; l < L; ++l) {
    lv.p[l] = (const __bf16*)levels[l];
    lv.H[l] = Hs[l];
    lv.W[l] = Ws[l];
  }
  const __bf16* a = (const __bf16*)f1;
  if (out_bf16) {
    return radius == 3
        ? alt_fwd_nc<3>(a, lv, coords, (__bf16*)out, BP, P, D, L, cl, ldc, stream)
        : alt_fwd_nc<4>(a, lv, coords, (__bf16*)out, BP, P, D, L, cl, ldc, stream);
  }
  return radius == 3
      ? alt_fwd_nc<3>(a, lv, coords, (float*)out, BP, P, D, L, cl, ldc, stream)
      : alt_fwd_nc<4>(a, lv, coords, (float*)out, BP, P, D, L, cl, ldc, stream);
}
