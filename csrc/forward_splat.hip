// Nearest-neighbour forward splat of a flow field onto the grid (the
// warm-start step of sequence inference; reference core/utils/utils.py:28-56,
// scipy griddata(method="nearest") there).
//
//   source i = y*W + x of sample b sits at (px, py) = (x + dx, y + dy), fp64;
//   valid iff 0 < px < W and 0 < py < H (NaN fails);
//   target (tx, ty) copies the (dx, dy) of the valid source with the smallest
//   d = (px-tx)^2 + (py-ty)^2 (fp64, products and sum rounded separately);
//   ties go to the lowest source index; no valid source -> zeros.
//
// Tiled brute force, two stages, no atomics. A workgroup owns FS_TILE
// targets of one sample and one chunk of that sample's sources. It stages
// the chunk FS_THREADS sources at a time into LDS as (px, py) doubles built
// from the fp32 flow; an invalid source is stored as +inf, so its distance
// is +inf and it never passes the strict `<` (no compaction pass). Every
// lane reads the same LDS address per step (a broadcast); each thread
// carries FS_TPT targets. Per-chunk (best d, best index) partials go to a
// workspace [B][G][H*W]; the finish kernel folds the chunks in ascending
// order with a strict `<` (sources ascend with the chunk number, so the
// lowest index still wins a tie), gathers the two flow values and writes
// the output. With G == 1 the search kernel writes the output itself.
//
// Nothing here depends on device data: grid, chunking and workspace come
// from (B, H, W, G) alone, so the launches are hipGraph-capturable and the
// result is bit-reproducible.

#include "common.h"

#include <limits>

#define FS_THREADS 256
#define FS_TPT 4
#define FS_TILE (FS_THREADS * FS_TPT)
// plan: aim for this many workgroups per sample, chunks no shorter than this
#define FS_TARGET_WGS 2048
#define FS_MIN_CHUNK 128

// d = ddx*ddx + ddy*ddy with each product and the sum rounded on its own:
// the contraction pragma keeps the compiler from fusing them into an FMA,
// so d rounds exactly like the fp64 oracle's.
__device__ __forceinline__ double fs_dist2(double ddx, double ddy) {
#pragma clang fp contract(off)
  const double a = ddx * ddx;
  const double b = ddy * ddy;
  return a + b;
}

template <bool DIRECT>
__global__ __launch_bounds__(FS_THREADS) void forward_splat_search_kernel(
    const float* __restrict__ flow,  // (B, 2, H, W)
    double* __restrict__ ws_d,       // (B, G, HW)   [!DIRECT]
    int* __restrict__ ws_i,          // (B, G, HW)   [!DIRECT]
    float* __restrict__ out,         // (B, 2, H, W) [DIRECT]
    int H, int W, int chunk) {
  const int HW = H * W;
  const int b = blockIdx.z;
  const int g = blockIdx.y;
  const int G = gridDim.y;
  const int t0 = blockIdx.x * FS_TILE + threadIdx.x;
  const float* fx = flow + (size_t)b * 2 * HW;
  const float* fy = fx + HW;

  double tx[FS_TPT], ty[FS_TPT], bd[FS_TPT];
  int bi[FS_TPT];
#pragma unroll
  for (int j = 0; j < FS_TPT; ++j) {
    const int t = t0 + j * FS_THREADS;  // past HW in the last tile: unused
    tx[j] = (double)(t % W);
    ty[j] = (double)(t / W);
    bd[j] = std::numeric_limits<double>::infinity();
    bi[j] = -1;
  }

  __shared__ double2 src[FS_THREADS];
  const int s0 = g * chunk;
  const int s1 = min(s0 + chunk, HW);
  for (int base = s0; base < s1; base += FS_THREADS) {
    const int i = base + threadIdx.x;
    double2 p;
    p.x = p.y = std::numeric_limits<double>::infinity();
    if (i < s1) {
      const double px = (double)(i % W) + (double)fx[i];
      const double py = (double)(i / W) + (double)fy[i];
      if (px > 0.0 && px < (double)W && py > 0.0 && py < (double)H) {
        p.x = px;
        p.y = py;
      }
    }
    __syncthreads();  // the previous pass has been read
    src[threadIdx.x] = p;
    __syncthreads();
    const int n = min(FS_THREADS, s1 - base);
    for (int k = 0; k < n; ++k) {
      const double2 q = src[k];
#pragma unroll
      for (int j = 0; j < FS_TPT; ++j) {
        const double ddx = q.x - tx[j];
        const double ddy = q.y - ty[j];
        const double d = fs_dist2(ddx, ddy);
        if (d < bd[j]) {
          bd[j] = d;
          bi[j] = base + k;
        }
      }
    }
  }

#pragma unroll
  for (int j = 0; j < FS_TPT; ++j) {
    const int t = t0 + j * FS_THREADS;
    if (t >= HW) continue;
    if (DIRECT) {
      float* o = out + (size_t)b * 2 * HW;
      o[t] = bi[j] >= 0 ? fx[bi[j]] : 0.0f;
      o[HW + t] = bi[j] >= 0 ? fy[bi[j]] : 0.0f;
    } else {
      const size_t w = ((size_t)b * G + g) * HW + t;
      ws_d[w] = bd[j];
      ws_i[w] = bi[j];
    }
  }
}

__global__ __launch_bounds__(FS_THREADS) void forward_splat_finish_kernel(
    const float* __restrict__ flow, const double* __restrict__ ws_d,
    const int* __restrict__ ws_i, float* __restrict__ out, int HW, int G) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * FS_THREADS + threadIdx.x;
  if (t >= HW) return;
  double bd = std::numeric_limits<double>::infinity();
  int bi = -1;
  for (int g = 0; g < G; ++g) {
    const size_t w = ((size_t)b * G + g) * HW + t;
    const double d = ws_d[w];
    if (d < bd) {
      bd = d;
      bi = ws_i[w];
    }
  }
  const float* fx = flow + (size_t)b * 2 * HW;
  float* o = out + (size_t)b * 2 * HW;
  o[t] = bi >= 0 ? fx[bi] : 0.0f;
  o[HW + t] = bi >= 0 ? fx[HW + bi] : 0.0f;
}

// Sources per chunk for `splits` requested chunks (0: planned), and the
// chunk count G that this chunk length gives (no empty chunk).
void flowhip_forward_splat_plan(int H, int W, int splits, int* chunk_out,
                                int* G_out) {
  const int HW = H * W;
  int G = splits;
  if (G <= 0) {
    const int tiles = fh_cdiv(HW, FS_TILE);
    G = fh_cdiv(FS_TARGET_WGS, tiles);
    const int gmax = HW / FS_MIN_CHUNK;
    if (G > gmax) G = gmax;
    if (G < 1) G = 1;
  }
  if (G > HW) G = HW;
  if (G > 65535) G = 65535;  // gridDim.y
  const int chunk = fh_cdiv(HW, G);
  *chunk_out = chunk;
  *G_out = fh_cdiv(HW, chunk);
}

// ws_d / ws_i: B*G*HW elements each, unused when G == 1.
void flowhip_forward_splat_launch(const float* flow, float* out, double* ws_d,
                                  int* ws_i, int B, int H, int W, int chunk,
                                  int G, hipStream_t stream) {
  const int HW = H * W;
  dim3 grid(fh_cdiv(HW, FS_TILE), G, B), block(FS_THREADS);
  if (G == 1) {
    hipLaunchKernelGGL(forward_splat_search_kernel<true>, grid, block, 0,
                       stream, flow, nullptr, nullptr, out, H, W, chunk);
    return;
  }
  hipLaunchKernelGGL(forward_splat_search_kernel<false>, grid, block, 0,
                     stream, flow, ws_d, ws_i, nullptr, H, W, chunk);
  hipLaunchKernelGGL(forward_splat_finish_kernel,
                     dim3(fh_cdiv(HW, FS_THREADS), B), block, 0, stream, flow,
                     ws_d, ws_i, out, HW, G);
}
