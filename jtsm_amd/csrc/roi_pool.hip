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
#include <cfloat>

#include "pool_bins.h"

namespace jtsm {
namespace {

#pragma clang fp contract(off)

// Per-roi record: image and the roi's rectangle.
struct PoolReach {
  int b;
  BinRect r;
  int pad;
};
static_assert(sizeof(PoolReach) == 32, "PoolReach is one 32-byte record");

__device__ __forceinline__ PoolReach pool_geometry(const float* __restrict__ roi, float scale, int PH, int PW) {
#pragma clang fp contract(off)
  const int x0 = (int)roundf(roi[1] * scale), y0 = (int)roundf(roi[2] * scale);
  const int x1 = (int)roundf(roi[3] * scale), y1 = (int)roundf(roi[4] * scale);
  return {(int)roi[0], BinRect(x0, y0, x1, y1, PH, PW), 0};
}

// One wavefront per (roi, bin row ph); lane owns channels [c, c + VEC) of every 64*VEC-channel block.
template <int VEC>
__global__ __launch_bounds__(256) void roi_pool_fwd_nhwc(const float* __restrict__ in, const float* __restrict__ rois,
                                                         float* __restrict__ out, int* __restrict__ argmax, int B, int C,
                                                         int H, int W, int R, float scale, int PH, int PW) {
#pragma clang fp contract(off)
  using V = typename VecT<VEC>::T;
  const long wave = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (wave >= (long)R * PH) return;
  const int lane = threadIdx.x & 63;
  const int n = (int)(wave / PH), ph = (int)(wave - (long)n * PH);
  const PoolReach g = pool_geometry(rois + (size_t)n * 5, scale, PH, PW);
  const bool ok = g.b >= 0 && g.b < B;            // (a roi naming no image pools nothing: 0 / -1)
  const float* __restrict__ img = in + (size_t)(ok ? g.b : 0) * H * W * C;
  const int hs = clampi(bin_lo(ph, g.r.bh, g.r.y0), 0, H), he = ok ? clampi(bin_hi(ph, g.r.bh, g.r.y0), 0, H) : 0;
  for (int c = lane * VEC; c < C; c += 64 * VEC) {
    for (int pw = 0; pw < PW; ++pw) {
      const size_t o = (((size_t)n * PH + ph) * PW + pw) * C + c;
      const int ws = clampi(bin_lo(pw, g.r.bw, g.r.x0), 0, W), we = clampi(bin_hi(pw, g.r.bw, g.r.x0), 0, W);
      const bool empty = he <= hs || we <= ws;
      V m;
      int a[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) { set_comp(m, k, empty ? 0.f : -FLT_MAX); a[k] = -1; }
      for (int h = hs; h < he; ++h) {
        const float* __restrict__ row = img + (size_t)h * W * C + c;
#pragma unroll 4
        for (int w = ws; w < we; ++w) {
          const V v = *reinterpret_cast<const V*>(row + (size_t)w * C);
          update_max<VEC>(v, h * W + w, m, a);
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
    const int hs = clampi(bin_lo(ph, g.r.bh, g.r.y0), 0, H), he = ok ? clampi(bin_hi(ph, g.r.bh, g.r.y0), 0, H) : 0;
    const int ws = clampi(bin_lo(pw, g.r.bw, g.r.x0), 0, W), we = clampi(bin_hi(pw, g.r.bw, g.r.x0), 0, W);
    const bool empty = he <= hs || we <= ws;
    float m = empty ? 0.f : -FLT_MAX;
    int a = -1;
    for (int h = hs; h < he; ++h)
      for (int w = ws; w < we; ++w) update_max(p[h * W + w], h * W + w, m, a);
    out[i] = m;
    argmax[i] = a;
  }
}

// (H, W: unused here — the reach kernels of both max pools take what the shared launcher passes.)
__global__ __launch_bounds__(256) void roi_pool_reach_kernel(const float* __restrict__ rois, PoolReach* __restrict__ reach,
                                                             int R, int H, int W, float scale, int PH, int PW) {
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
  using V = typename VecT<VEC>::T;
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
    if (q.b != b || !q.r.reaches(h, w)) continue;
    for_bins_holding(q.r, h, w, PH, PW, [&](int ph, int pw) {
      if (live) gather_add<VEC>(acc, grad, argmax, ((size_t)n * PH + ph) * PW + pw, C, c, idx);
    });
  }
  if (!live) return;
  V v;
#pragma unroll
  for (int k = 0; k < VEC; ++k) set_comp(v, k, acc[k]);
  *reinterpret_cast<V*>(gin + (size_t)cell * C + c) = v;
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" {

int jtsm_roi_pool_forward_f32(const float* input, const float* rois, float* output, int32_t* argmax, int B, int C, int H,
                              int W, int R, float spatial_scale, int pooled_h, int pooled_w, int layout, void* stream) {
  return pool_forward<roi_pool_fwd_nhwc<4>, roi_pool_fwd_nhwc<1>, roi_pool_fwd_nchw>(
      "roi_pool", input, rois, output, argmax, B, C, H, W, R, spatial_scale, pooled_h, pooled_w, layout, stream);
}

size_t jtsm_roi_pool_backward_workspace_bytes(int R) { return pool_backward_workspace_bytes<PoolReach>(R); }

int jtsm_roi_pool_backward_f32(const float* grad, const float* rois, const int32_t* argmax, float* grad_input,
                               void* workspace, int B, int C, int H, int W, int R, float spatial_scale, int pooled_h,
                               int pooled_w, void* stream) {
  return pool_backward<PoolReach, roi_pool_reach_kernel, roi_pool_bwd_gather<4>, roi_pool_bwd_gather<1>>(
      "roi_pool", grad, rois, argmax, grad_input, workspace, B, C, H, W, R, spatial_scale, pooled_h, pooled_w, stream);
}

}  // extern "C"
