// Fused convex-combination x8 upsample (kernel #11 of SURVEY.md §2.2) —
// the RAFT baseline's learned upsampler (reference core/raft.py:73-84).
//
//   out[n, c, 8y+sy, 8x+sx] = sum_k softmax(mask[n, :, sy, sx, y, x])[k]
//                                   * 8*flow[n, c, y+ky-1, x+kx-1]
// with k = ky*3+kx over the 3x3 neighborhood (zero-padded, F.unfold order)
// and mask channel layout ch = (k*8 + sy)*8 + sx (the reference's
// view(N,1,9,8,8,H,W)).
//
// The reference materializes softmax(mask) (N,9,64,H,W) and the unfold
// product at full resolution; this kernel reads mask+flow once and writes
// the output once. Backward: dmask is per-output-pixel exclusive (no
// atomics); dflow gathers 576 contributions per coarse pixel via fp32
// atomicAdd (each add L2-local).
//
// Deterministic backward (DET = true, flowhip.ops.set_deterministic): the
// thread layout, and with it dmask's arithmetic, stay the same. The 8 lanes
// that share (n, oy, x) add their 9x2 products w_k * g_c with a 3-step xor
// butterfly and write them once to contrib (N, H, W, 8 sy, 9, 2);
// convex_up_gflow_gather_kernel then sums, per coarse pixel and channel, the
// 9 neighbours' 8 rows in ascending (k, sy). No atomics, no zero fill, the
// order fixed by indices alone.

#include "common.h"

#define CU_THREADS 256

template <int F>
__global__ __launch_bounds__(CU_THREADS) void convex_up_fwd_kernel(
    const float* __restrict__ flow,  // (N, 2, H, W)
    const float* __restrict__ mask,  // (N, 9*F*F, H, W)
    float* __restrict__ out,         // (N, 2, F*H, F*W)
    int N, int H, int W) {
  const long total = (long)N * F * H * F * W;
  const long idx0 = (long)blockIdx.x * CU_THREADS + threadIdx.x;
  if (idx0 >= total) return;

  // decode (n, oy, ox); adjacent threads = adjacent ox (coalesced store)
  long t = idx0;
  const int ox = t % (F * W); t /= (F * W);
  const int oy = t % (F * H); t /= (F * H);
  const int n = t;

  const int x = ox / F, sx = ox % F;
  const int y = oy / F, sy = oy % F;
  const long P = (long)H * W;

  // softmax over the 9 mask logits for this subpixel
  const float* mbase = mask + ((long)n * 9 * F * F) * P + (long)y * W + x;
  float logits[9];
  float mx = -1e30f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    logits[k] = mbase[(long)((k * F + sy) * F + sx) * P];
    mx = fmaxf(mx, logits[k]);
  }
  float wsum = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    logits[k] = __expf(logits[k] - mx);
    wsum += logits[k];
  }
  const float inv = 1.0f / wsum;

  const float* fbase = flow + (long)n * 2 * P;
  float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int yy = y + ky - 1, xx = x + kx - 1;
      if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
      const float w = logits[ky * 3 + kx] * inv;
      acc0 += w * fbase[(long)yy * W + xx];
      acc1 += w * fbase[P + (long)yy * W + xx];
    }
  }
  float* obase = out + (long)n * 2 * F * H * F * W;
  obase[(long)oy * F * W + ox] = 8.0f * acc0;
  obase[(long)F * H * F * W + (long)oy * F * W + ox] = 8.0f * acc1;
}

template <int F, bool DET>
__global__ __launch_bounds__(CU_THREADS) void convex_up_bwd_kernel(
    const float* __restrict__ gout,  // (N, 2, F*H, F*W)
    const float* __restrict__ flow,  // (N, 2, H, W)
    const float* __restrict__ mask,  // (N, 9*F*F, H, W)
    float* __restrict__ gflow,       // !DET: (N, 2, H, W) zero-init, atomic
                                     // DET: contrib (N, H, W, F, 9, 2)
    float* __restrict__ gmask,       // (N, 9*F*F, H, W)
    int N, int H, int W) {
  static_assert(!DET || F == 8, "the butterfly spans 8 sub-pixel lanes");
  const long total = (long)N * F * H * F * W;
  const long idx0 = (long)blockIdx.x * CU_THREADS + threadIdx.x;
  // total is a multiple of 64: a wave leaves whole, so every lane of the
  // DET butterfly below is live
  if (idx0 >= total) return;

  long t = idx0;
  const int ox = t % (F * W); t /= (F * W);
  const int oy = t % (F * H); t /= (F * H);
  const int n = t;

  const int x = ox / F, sx = ox % F;
  const int y = oy / F, sy = oy % F;
  const long P = (long)H * W;

  const float* mbase = mask + ((long)n * 9 * F * F) * P + (long)y * W + x;
  float w[9];
  float mx = -1e30f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    w[k] = mbase[(long)((k * F + sy) * F + sx) * P];
    mx = fmaxf(mx, w[k]);
  }
  float wsum = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    w[k] = __expf(w[k] - mx);
    wsum += w[k];
  }
  const float inv = 1.0f / wsum;
#pragma unroll
  for (int k = 0; k < 9; ++k) w[k] *= inv;

  const float* fbase = flow + (long)n * 2 * P;
  const float* gbase = gout + (long)n * 2 * F * H * F * W;
  const float g0 = 8.0f * gbase[(long)oy * F * W + ox];
  const float g1 = 8.0f * gbase[(long)F * H * F * W + (long)oy * F * W + ox];

  // dw_k = sum_c g_c * f_k[c];  dm_k = w_k * (dw_k - sum_j w_j dw_j)
  float dw[9];
  float dot = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int k = ky * 3 + kx;
      const int yy = y + ky - 1, xx = x + kx - 1;
      float f0 = 0.f, f1 = 0.f;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
        f0 = fbase[(long)yy * W + xx];
        f1 = fbase[P + (long)yy * W + xx];
        if constexpr (!DET) {
          // dflow: scatter the weighted grad into the neighborhood
          atomicAdd((float*)&gflow[(long)n * 2 * P + (long)yy * W + xx],
                    w[k] * g0);
          atomicAdd((float*)&gflow[(long)n * 2 * P + P + (long)yy * W + xx],
                    w[k] * g1);
        }
      }
      dw[k] = g0 * f0 + g1 * f1;
      dot += w[k] * dw[k];
    }
  }
  float* gm = gmask + ((long)n * 9 * F * F) * P + (long)y * W + x;
#pragma unroll
  for (int k = 0; k < 9; ++k)
    gm[(long)((k * F + sy) * F + sx) * P] = w[k] * (dw[k] - dot);

  if constexpr (DET) {
    // F*W and the block size are multiples of 8, so the 8 lanes of one
    // (n, oy, x) are an aligned lane group: sx == lane & 7. Every tap is
    // stored, also one whose neighbour lies outside the map; the gather
    // kernel never reads those.
    float* cb = gflow + ((((long)n * H + y) * W + x) * F + sy) * 18;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float v = w[k] * (c ? g1 : g0);
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 4);
        if (sx == ((k * 2 + c) & 7)) cb[k * 2 + c] = v;
      }
    }
  }
}

// gflow[n, c, y, x] = sum_k sum_sy contrib[n, y-(ky-1), x-(kx-1), sy, k, c]
// in ascending (k, sy); a neighbour outside the map contributes nothing.
__global__ __launch_bounds__(CU_THREADS) void convex_up_gflow_gather_kernel(
    const float* __restrict__ contrib,  // (N, H, W, 8, 9, 2)
    float* __restrict__ gflow,          // (N, 2, H, W)
    int N, int H, int W) {
  const long total = (long)N * 2 * H * W;
  const long idx = (long)blockIdx.x * CU_THREADS + threadIdx.x;
  if (idx >= total) return;
  long t = idx;
  const int x = t % W; t /= W;
  const int y = t % H; t /= H;
  const int c = t % 2; t /= 2;
  const int n = t;
  float acc = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ys = y - (ky - 1), xs = x - (kx - 1);
      if (ys < 0 || ys >= H || xs < 0 || xs >= W) continue;
      const float* cb = contrib + (((long)n * H + ys) * W + xs) * (8 * 18) +
                        (ky * 3 + kx) * 2 + c;
#pragma unroll
      for (int sy = 0; sy < 8; ++sy) acc += cb[sy * 18];
    }
  }
  gflow[idx] = acc;
}

void flowhip_convex_up_fwd_launch(const float* flow, const float* mask,
                                  float* out, int N, int H, int W, int factor,
                                  hipStream_t stream) {
  if (factor != 8) abort();
  const long total = (long)N * 8 * H * 8 * W;
  dim3 grid((unsigned)((total + CU_THREADS - 1) / CU_THREADS));
  hipLaunchKernelGGL((convex_up_fwd_kernel<8>), grid, dim3(CU_THREADS), 0,
                     stream, flow, mask, out, N, H, W);
}

// contrib == nullptr: the atomic form, gflow zero-filled by the caller.
// Otherwise the deterministic form: contrib holds N*H*W*8*9*2 floats, all
// written before they are read, and gflow needs no fill.
void flowhip_convex_up_bwd_launch(const float* gout, const float* flow,
                                  const float* mask, float* gflow,
                                  float* gmask, float* contrib, int N, int H,
                                  int W, int factor, hipStream_t stream) {
  if (factor != 8) abort();
  const long total = (long)N * 8 * H * 8 * W;
  dim3 grid((unsigned)((total + CU_THREADS - 1) / CU_THREADS));
  if (contrib) {
    hipLaunchKernelGGL((convex_up_bwd_kernel<8, true>), grid,
                       dim3(CU_THREADS), 0, stream, gout, flow, mask, contrib,
                       gmask, N, H, W);
    const long cells = (long)N * 2 * H * W;
    hipLaunchKernelGGL(convex_up_gflow_gather_kernel,
                       dim3((unsigned)((cells + CU_THREADS - 1) / CU_THREADS)),
                       dim3(CU_THREADS), 0, stream, contrib, gflow, N, H, W);
    return;
  }
  hipLaunchKernelGGL((convex_up_bwd_kernel<8, false>), grid, dim3(CU_THREADS),
                     0, stream, gout, flow, mask, gflow, gmask, N, H, W);
}
