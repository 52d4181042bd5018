// ROIPool for gfx950 — the plain ROI max-pool PCL's box head reads (POOLER_TYPE "ROIPool").
//
// Replaces torchvision.ops.RoIPool as the reference calls it (projects/WSL/wsl/modeling/poolers.py:6,183-186:
// RoIPool(output_size, spatial_scale)(input, rois) -> output; the operator keeps an int argmax for its backward).
//
// Contract.  rois (R,5) = (b, x1, y1, x2, y2); output / argmax (R, C, PH, PW).  Per roi:
//   integer rectangle: roundf(coord * scale) (half away from zero)
//   roi_w = max(x_end - x_start + 1, 1), roi_h likewise; bin = (float)roi_w / PW, (float)roi_h / PH
//   bin p covers [floor(p*bin), ceil((p+1)*bin)) + start, clipped to [0, W] / [0, H]
//   an empty bin gives 0 / -1; otherwise the maximum starts at -FLT_MAX (argmax -1) and the bin is scanned h outer,
//   w inner with a strict '>': the first cell holding the maximum wins
//   argmax: flat h*W + w in the (image, channel) plane.
// Backward: grad_in[b, c, argmax] += grad_out[n, c, ph, pw] wherever argmax >= 0.
//
// Forward (NHWC): one wavefront per (roi, bin row); lanes hold channels (4 floats each: 1 KiB per 256-channel row).
// NCHW: one thread per (roi, channel, bin).
// Backward (NHWC): a GATHER, as ROILoopPool's — one wavefront per (image, cell) and 256-channel block walks the rois in
// index order, finds the bins that hold the cell from the integer geometry alone (precomputed per roi by a small
// kernel) and adds the gradients whose argmax names the cell.  Every cell is written once, no atomics: two calls on
// the same inputs give the same bits.
#include <algorithm>
#include <cfloat>

#include "common.h"

namespace jtsm {
namespace {

#pragma clang fp contract(off)

__device__ __forceinline__ int rp_clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// Per-roi record: image, rectangle start, unclipped reach [start, start + ceil(P * bin)), bin sizes.
struct PoolReach {
  int b, x0, y0, xe, ye;
  float bw, bh;
  int pad;
};
static_assert(sizeof(PoolReach) == 32, "PoolReach is one 32-byte record");

__device__ __forceinline__ int rp_bin_lo(int p, float bin, int s) { return (int)floorf((float)p * bin) + s; }
__device__ __forceinline__ int rp_bin_hi(int p, float bin, int s) { return (int)ceilf((float)(p + 1) * bin) + s; }

__device__ __forceinline__ PoolReach pool_geometry(const float* __restrict__ roi, float scale, int PH, int PW) {
#pragma clang fp contract(off)
  PoolReach q;
  q.b = (int)roi[0];
  q.x0 = (int)roundf(roi[1] * scale);
  q.y0 = (int)roundf(roi[2] * scale);
  const int x1 = (int)roundf(roi[3] * scale), y1 = (int)roundf(roi[4] * scale);
  q.bw = (float)max(x1 - q.x0 + 1, 1) / (float)PW;
  q.bh = (float)max(y1 - q.y0 + 1, 1) / (float)PH;
  q.xe = rp_bin_hi(PW - 1, q.bw, q.x0);
  q.ye = rp_bin_hi(PH - 1, q.bh, q.y0);
  q.pad = 0;
  return q;
}

template <int VEC> struct RpVec;
template <> struct RpVec<4> { using T = float4; };
template <> struct RpVec<1> { using T = float; };

__device__ __forceinline__ float rp_comp(const float4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
__device__ __forceinline__ float rp_comp(const float& v, int) { return v; }
__device__ __forceinline__ void rp_set(float4& v, int k, float x) {
  if (k == 0) v.x = x; else if (k == 1) v.y = x; else if (k == 2) v.z = x; else v.w = x;
}
__device__ __forceinline__ void rp_set(float& v, int, float x) { v = x; }

// One wavefront per (roi, bin row ph); lane owns channels [c, c + VEC) of every 64*VEC-channel block.
template <int VEC>
__global__ __launch_bounds__(256) void roi_pool_fwd_nhwc(const float* __restrict__ in, const float* __restrict__ rois,
                                                         float* __restrict__ out, int* __restrict__ argmax, int B, int C,
                                                         int H, int W, int R, float scale, int PH, int PW) {
#pragma clang fp contract(off)
  using V = typename RpVec<VEC>::T;
  const long wave = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (wave >= (long)R * PH) return;
  const int lane = threadIdx.x & 63;
  const int n = (int)(wave / PH), ph = (int)(wave - (long)n * PH);
  const PoolReach g = pool_geometry(rois + (size_t)n * 5, scale, PH, PW);
  const bool ok = g.b >= 0 && g.b < B;            // (a roi naming no image pools nothing: 0 / -1)
  const float* __restrict__ img = in + (size_t)(ok ? g.b : 0) * H * W * C;
  const int hs = rp_clampi(rp_bin_lo(ph, g.bh, g.y0), 0, H), he = ok ? rp_clampi(rp_bin_hi(ph, g.bh, g.y0), 0, H) : 0;
  for (int c = lane * VEC; c < C; c += 64 * VEC) {
    for (int pw = 0; pw < PW; ++pw) {
      const size_t o = (((size_t)n * PH + ph) * PW + pw) * C + c;
      const int ws = rp_clampi(rp_bin_lo(pw, g.bw, g.x0), 0, W), we = rp_clampi(rp_bin_hi(pw, g.bw, g.x0), 0, W);
      const bool empty = he <= hs || we <= ws;
      V m;
      int a[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) { rp_set(m, k, empty ? 0.f : -FLT_MAX); a[k] = -1; }
      for (int h = hs; h < he; ++h) {
        const float* __restrict__ row = img + (size_t)h * W * C + c;
#pragma unroll 4
        for (int w = ws; w < we; ++w) {
          const V v = *reinterpret_cast<const V*>(row + (size_t)w * C);
          const int idx = h * W + w;
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            const float x = rp_comp(v, k);
            if (x > rp_comp(m, k)) { rp_set(m, k, x); a[k] = idx; }
          }
        }
      }
      *reinterpret_cast<V*>(out + o) = m;
#pragma unroll
      for (int k = 0; k < VEC; ++k) argmax[o + k] = a[k];
    }
  }
}

// NCHW: one thread per (roi, channel, bin).
__global__ __launch_bounds__(256) void roi_pool_fwd_nchw(const float* __restrict__ in, const float* __restrict__ rois,
                                                         float* __restrict__ out, int* __restrict__ argmax, int B, int C,
                                                         int H, int W, int R, float scale, int PH, int PW) {
#pragma clang fp contract(off)
  const long total = (long)R * C * PH * PW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int pw = (int)(i % PW), ph = (int)((i / PW) % PH), c = (int)((i / PW / PH) % C), n = (int)(i / PW / PH / C);
    const PoolReach g = pool_geometry(rois + (size_t)n * 5, scale, PH, PW);
    const bool ok = g.b >= 0 && g.b < B;
    const float* __restrict__ p = in + ((size_t)(ok ? g.b : 0) * C + c) * H * W;
    const int hs = rp_clampi(rp_bin_lo(ph, g.bh, g.y0), 0, H), he = ok ? rp_clampi(rp_bin_hi(ph, g.bh, g.y0), 0, H) : 0;
    const int ws = rp_clampi(rp_bin_lo(pw, g.bw, g.x0), 0, W), we = rp_clampi(rp_bin_hi(pw, g.bw, g.x0), 0, W);
    const bool empty = he <= hs || we <= ws;
    float m = empty ? 0.f : -FLT_MAX;
    int a = -1;
    for (int h = hs; h < he; ++h)
      for (int w = ws; w < we; ++w) {
        const int idx = h * W + w;
        const float x = p[idx];
        if (x > m) { m = x; a = idx; }
      }
    out[i] = m;
    argmax[i] = a;
  }
}

__global__ __launch_bounds__(256) void roi_pool_reach_kernel(const float* __restrict__ rois, PoolReach* __restrict__ reach,
                                                             int R, float scale, int PH, int PW) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= R) return;
  reach[n] = pool_geometry(rois + (size_t)n * 5, scale, PH, PW);
}

// grad_in[b, h, w, c] = sum over (roi n, bin (ph, pw)) whose bin holds (h, w) and whose argmax names it of
// grad[n, ph, pw, c] — roi order, then bin: a fixed order.  One wavefront per (image, cell) and 64*VEC-channel block
// (grid.y).
template <int VEC>
__global__ __launch_bounds__(256) void roi_pool_bwd_gather(const float* __restrict__ grad, const int* __restrict__ argmax,
                                                           const PoolReach* __restrict__ reach, float* __restrict__ gin,
                                                           int B, int C, int H, int W, int R, int PH, int PW) {
#pragma clang fp contract(off)
  using V = typename RpVec<VEC>::T;
  const long cell = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (cell >= (long)B * H * W) return;
  const int lane = threadIdx.x & 63;
  const int w = (int)(cell % W), h = (int)((cell / W) % H), b = (int)(cell / W / H);
  const int c = (blockIdx.y * 64 + lane) * VEC;
  const bool live = c < C;
  const int idx = h * W + w;
  float acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
  for (int n = 0; n < R; ++n) {
    const PoolReach q = reach[n];   // (uniform: scalar loads)
    if (q.b != b || h < q.y0 || h >= q.ye || w < q.x0 || w >= q.xe) continue;
    for (int ph = 0; ph < PH; ++ph) {
      if (h < rp_bin_lo(ph, q.bh, q.y0) || h >= rp_bin_hi(ph, q.bh, q.y0)) continue;
      for (int pw = 0; pw < PW; ++pw) {
        if (w < rp_bin_lo(pw, q.bw, q.x0) || w >= rp_bin_hi(pw, q.bw, q.x0)) continue;
        if (!live) continue;
        const size_t o = (((size_t)n * PH + ph) * PW + pw) * C + c;
#pragma unroll
        for (int k = 0; k < VEC; ++k)
          if (argmax[o + k] == idx) acc[k] += grad[o + k];
      }
    }
  }
  if (!live) return;
  V v;
#pragma unroll
  for (int k = 0; k < VEC; ++k) rp_set(v, k, acc[k]);
  *reinterpret_cast<V*>(gin + (size_t)cell * C + c) = v;
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" {

int jtsm_roi_pool_forward_f32(const float* input, const float* rois, float* output, int32_t* argmax, int B, int C, int H,
                              int W, int R, float spatial_scale, int pooled_h, int pooled_w, int layout, void* stream) {
  JTSM_REQUIRE(B >= 0 && C >= 0 && H >= 0 && W >= 0 && R >= 0 && pooled_h > 0 && pooled_w > 0, "roi_pool: negative size");
  JTSM_REQUIRE(layout == JTSM_NCHW || layout == JTSM_NHWC, "roi_pool: unknown layout %d", layout);
  if ((long)R * C == 0) return JTSM_OK;
  JTSM_REQUIRE(input && rois && output && argmax, "roi_pool: null pointer");
  JTSM_REQUIRE(B > 0 && H > 0 && W > 0, "roi_pool: empty feature map");
  JTSM_REQUIRE((long)H * W < (1L << 31), "roi_pool: map too large for int32 argmax");
  hipStream_t st = as_stream(stream);
  if (layout == JTSM_NHWC) {
    const int blocks = ceil_div((long)R * pooled_h, 4);
    const bool v4 = C % 4 == 0 && ((uintptr_t)input & 15) == 0 && ((uintptr_t)output & 15) == 0;
    if (v4)
      hipLaunchKernelGGL(roi_pool_fwd_nhwc<4>, dim3(blocks), dim3(256), 0, st, input, rois, output, argmax, B, C, H, W, R,
                         spatial_scale, pooled_h, pooled_w);
    else
      hipLaunchKernelGGL(roi_pool_fwd_nhwc<1>, dim3(blocks), dim3(256), 0, st, input, rois, output, argmax, B, C, H, W, R,
                         spatial_scale, pooled_h, pooled_w);
  } else {
    const long total = (long)R * C * pooled_h * pooled_w;
    const int blocks = (int)std::min<long>(ceil_div(total, 256), 8192);
    hipLaunchKernelGGL(roi_pool_fwd_nchw, dim3(blocks), dim3(256), 0, st, input, rois, output, argmax, B, C, H, W, R,
                       spatial_scale, pooled_h, pooled_w);
  }
  JTSM_CHECK_LAUNCH("roi_pool forward");
  return JTSM_OK;
}

size_t jtsm_roi_pool_backward_workspace_bytes(int R) { return R > 0 ? (size_t)R * sizeof(PoolReach) : 16; }

int jtsm_roi_pool_backward_f32(const float* grad, const float* rois, const int32_t* argmax, float* grad_input,
                               void* workspace, int B, int C, int H, int W, int R, float spatial_scale, int pooled_h,
                               int pooled_w, void* stream) {
  JTSM_REQUIRE(B >= 0 && C >= 0 && H >= 0 && W >= 0 && R >= 0 && pooled_h > 0 && pooled_w > 0,
               "roi_pool backward: negative size");
  const long cells = (long)B * H * W;
  if (cells * C == 0) return JTSM_OK;
  JTSM_REQUIRE(grad_input && workspace, "roi_pool backward: null grad_input / workspace");
  JTSM_REQUIRE(R == 0 || (grad && rois && argmax), "roi_pool backward: null pointer");
  JTSM_REQUIRE(((uintptr_t)workspace & 15) == 0, "roi_pool backward: workspace must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  PoolReach* reach = reinterpret_cast<PoolReach*>(workspace);
  if (R > 0)
    hipLaunchKernelGGL(roi_pool_reach_kernel, dim3(ceil_div(R, 256)), dim3(256), 0, st, rois, reach, R, spatial_scale,
                       pooled_h, pooled_w);
  const bool v4 = C % 4 == 0 && ((uintptr_t)grad_input & 15) == 0 && ((uintptr_t)grad & 15) == 0;
  const int vec = v4 ? 4 : 1;
  const dim3 grid(ceil_div(cells, 4), ceil_div(C, 64 * vec));
  if (v4)
    hipLaunchKernelGGL(roi_pool_bwd_gather<4>, grid, dim3(256), 0, st, grad, argmax, reach, grad_input, B, C, H, W, R,
                       pooled_h, pooled_w);
  else
    hipLaunchKernelGGL(roi_pool_bwd_gather<1>, grid, dim3(256), 0, st, grad, argmax, reach, grad_input, B, C, H, W, R,
                       pooled_h, pooled_w);
  JTSM_CHECK_LAUNCH("roi_pool backward");
  return JTSM_OK;
}

}  // extern "C"
