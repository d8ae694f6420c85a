// Forward-backward consistency check of a bidirectional flow pair (the
// UnFlow occlusion test; twin: ops/torch_ref.py:fb_consistency).
//
//   one direction, f checked against b, fp64 on the fp32 inputs:
//   p   = (x + f_x, y + f_y); in frame iff 0 <= p_x <= W-1, 0 <= p_y <= H-1
//   b~  = bilinear sample of b at p, x0 = min(floor(p_x), W-2), w_x = p_x - x0
//   r2  = |f + b~|^2,  thr = alpha1 * (|f|^2 + |b~|^2) + alpha2
//   visible iff in frame, r2 and thr finite, r2 <= thr
//   occ = !visible (uint8), res = sqrt(r2) (fp32; +inf where not finite or
//   out of frame), stats = {visible, inconsistent, out/non-finite, sum res}
//
// One launch covers both directions: blockIdx.z picks which flow is f and
// which is b. Pixels are indexed flat over the H*W plane, lanes along x, so
// the f loads and every store are coalesced. One pixel per thread: a form
// with 4 consecutive pixels per thread (16-byte f loads, 4-byte occ stores)
// measured 1.4x slower at 1088x1920 and no faster at 288x960
// (profiles/README.md), so the simpler form stayed.
// The in-frame test is done on the fp64 position before anything becomes an
// int: a lane that fails it (NaN, +-inf, 1e30 included) loads nothing.
//
// Every operation of the decision is rounded on its own (contraction off),
// so it rounds like the fp64 twin. stats is a two-stage reduction in a fixed
// order, no atomics: per-workgroup partials, then one workgroup per (sample,
// direction) folds them. Grid and workspace come from (N, H, W) alone: no
// host sync, hipGraph-capturable, bit-reproducible.

#include "common.h"

#include <limits>

#define FB_THREADS 256
#define FB_WAVES (FB_THREADS / 64)

struct FbAcc {
  double vis, inc, out, sum;
};

// Class of one pixel (0 visible, 1 in frame but inconsistent, 2 out of frame
// or non-finite) and its residual.
__device__ __forceinline__ int fb_pixel(const float* __restrict__ bx,
                                        const float* __restrict__ by,
                                        float fxv, float fyv, int x, int y,
                                        int H, int W, double a1, double a2,
                                        float* res, double* r) {
#pragma clang fp contract(off)
  const double fx = (double)fxv, fy = (double)fyv;
  const double px = (double)x + fx;
  const double py = (double)y + fy;
  *res = std::numeric_limits<float>::infinity();
  *r = 0.0;
  const bool in = px >= 0.0 && px <= (double)(W - 1) && py >= 0.0 &&
                  py <= (double)(H - 1);
  if (!in) return 2;
  // in frame: 0 <= floor(p) <= W-1 fits an int; every tap is inside b
  const int x0 = min((int)floor(px), W - 2);
  const int y0 = min((int)floor(py), H - 2);
  const double wx = px - (double)x0, wy = py - (double)y0;
  const double ux = 1.0 - wx, uy = 1.0 - wy;
  const int i00 = y0 * W + x0;
  const double tx = (double)bx[i00] * ux + (double)bx[i00 + 1] * wx;
  const double ty = (double)by[i00] * ux + (double)by[i00 + 1] * wx;
  const double lx = (double)bx[i00 + W] * ux + (double)bx[i00 + W + 1] * wx;
  const double ly = (double)by[i00 + W] * ux + (double)by[i00 + W + 1] * wx;
  const double sbx = tx * uy + lx * wy;
  const double sby = ty * uy + ly * wy;
  const double sx = fx + sbx, sy = fy + sby;
  const double r2 = sx * sx + sy * sy;
  const double thr = a1 * ((fx * fx + fy * fy) + (sbx * sbx + sby * sby)) + a2;
  if (!(isfinite(r2) && isfinite(thr))) return 2;
  const double root = sqrt(r2);
  *res = (float)root;
  if (r2 <= thr) {
    *r = root;
    return 0;
  }
  return 1;
}

// Fixed-order workgroup reduction of the four accumulators; thread 0 ends
// with the totals.
__device__ __forceinline__ FbAcc fb_block_reduce(FbAcc a) {
  __shared__ double red[FB_WAVES][4];
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) {
    a.vis += __shfl_down(a.vis, sh, 64);
    a.inc += __shfl_down(a.inc, sh, 64);
    a.out += __shfl_down(a.out, sh, 64);
    a.sum += __shfl_down(a.sum, sh, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[wave][0] = a.vis;
    red[wave][1] = a.inc;
    red[wave][2] = a.out;
    red[wave][3] = a.sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.vis = a.inc = a.out = a.sum = 0.0;
    for (int w = 0; w < FB_WAVES; ++w) {
      a.vis += red[w][0];
      a.inc += red[w][1];
      a.out += red[w][2];
      a.sum += red[w][3];
    }
  }
  return a;
}

// grid (ceil(HW / FB_THREADS), N, 2), one pixel per thread.
__global__ __launch_bounds__(FB_THREADS) void fb_consistency_kernel(
    const float* __restrict__ flow_fw,  // (N, 2, H, W)
    const float* __restrict__ flow_bw,  // (N, 2, H, W)
    unsigned char* __restrict__ occ,    // (2, N, H, W)  dir-major
    float* __restrict__ res,            // (2, N, H, W)
    double* __restrict__ partials,      // (2, N, gridDim.x, 4)
    int H, int W, double a1, double a2) {
  const int HW = H * W;
  const int n = blockIdx.y, N = gridDim.y;
  const int dir = blockIdx.z;
  const float* f = (dir == 0 ? flow_fw : flow_bw) + (size_t)n * 2 * HW;
  const float* b = (dir == 0 ? flow_bw : flow_fw) + (size_t)n * 2 * HW;
  const size_t plane = ((size_t)dir * N + n) * HW;

  // gridDim.x * FB_THREADS < HW + FB_THREADS stays inside int: the binding
  // keeps HW below 2^31 - 4096
  const int i = blockIdx.x * FB_THREADS + threadIdx.x;
  FbAcc acc = {0.0, 0.0, 0.0, 0.0};
  if (i < HW) {
    float r32;
    double r;
    const int cls = fb_pixel(b, b + HW, f[i], f[HW + i], i % W, i / W, H, W,
                             a1, a2, &r32, &r);
    occ[plane + i] = cls != 0;
    res[plane + i] = r32;
    acc.vis = cls == 0 ? 1.0 : 0.0;
    acc.inc = cls == 1 ? 1.0 : 0.0;
    acc.out = cls == 2 ? 1.0 : 0.0;
    acc.sum = r;
  }

  acc = fb_block_reduce(acc);
  if (threadIdx.x == 0) {
    double* p =
        partials + (((size_t)dir * N + n) * gridDim.x + blockIdx.x) * 4;
    p[0] = acc.vis;
    p[1] = acc.inc;
    p[2] = acc.out;
    p[3] = acc.sum;
  }
}

// grid (N, 2): folds the `nblk` partials of one (sample, direction), thread
// t taking blocks t, t + FB_THREADS, ... in ascending order.
__global__ __launch_bounds__(FB_THREADS) void fb_consistency_stats_kernel(
    const double* __restrict__ partials, double* __restrict__ stats,  // (N,2,4)
    int nblk) {
  const int n = blockIdx.x, N = gridDim.x;
  const int dir = blockIdx.y;
  const double* p = partials + ((size_t)dir * N + n) * nblk * 4;
  FbAcc acc = {0.0, 0.0, 0.0, 0.0};
  for (int k = threadIdx.x; k < nblk; k += FB_THREADS) {
    acc.vis += p[(size_t)k * 4 + 0];
    acc.inc += p[(size_t)k * 4 + 1];
    acc.out += p[(size_t)k * 4 + 2];
    acc.sum += p[(size_t)k * 4 + 3];
  }
  acc = fb_block_reduce(acc);
  if (threadIdx.x == 0) {
    double* s = stats + ((size_t)n * 2 + dir) * 4;
    s[0] = acc.vis;
    s[1] = acc.inc;
    s[2] = acc.out;
    s[3] = acc.sum;
  }
}

// Workgroups per (sample, direction).
int flowhip_fb_consistency_blocks(int H, int W) {
  return fh_cdiv(H * W, FB_THREADS);
}

// occ / res: (2, N, H, W) direction-major; partials: 2*N*blocks*4 doubles;
// stats: (N, 2, 4).
void flowhip_fb_consistency_launch(const float* flow_fw, const float* flow_bw,
                                   unsigned char* occ, float* res,
                                   double* partials, double* stats, int N,
                                   int H, int W, double alpha1, double alpha2,
                                   hipStream_t stream) {
  const int nblk = flowhip_fb_consistency_blocks(H, W);
  dim3 grid(nblk, N, 2), block(FB_THREADS);
  hipLaunchKernelGGL(fb_consistency_kernel, grid, block, 0, stream, flow_fw,
                     flow_bw, occ, res, partials, H, W, alpha1, alpha2);
  hipLaunchKernelGGL(fb_consistency_stats_kernel, dim3(N, 2), block, 0, stream,
                     partials, stats, nblk);
}
