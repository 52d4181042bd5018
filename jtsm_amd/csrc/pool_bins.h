// What ROIPool (roi_pool.hip) and ROILoopPool (roi_loop_pool.hip) have in common: the bin arithmetic of a max pool over
// an integer rectangle, the per-lane channel vector, the strict-'>' maximum update, the backward gather's "which bins
// hold this cell" walk, and the host side of the two entry points.  Nothing here knows which operator calls it: the
// operators' contracts (start value, blocks, frame mask, context skip) live in their own kernels.
#pragma once
#include <algorithm>

#include "common.h"

namespace jtsm {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// bin size of a rectangle [s, e] over P bins (ROILoopPool_cuda.cu:88-91; RoIPool's max(end - start + 1, 1) / P likewise)
__device__ __forceinline__ float bin_size(int s, int e, int P) {
#pragma clang fp contract(off)
  return (float)max(e - s + 1, 1) / (float)P;
}
// unclipped [lo, hi) of bin p (the clip to the map is applied by the callers that scan)
__device__ __forceinline__ int bin_lo(int p, float bin, int s) {
#pragma clang fp contract(off)
  return (int)floorf((float)p * bin) + s;
}
__device__ __forceinline__ int bin_hi(int p, float bin, int s) {
#pragma clang fp contract(off)
  return (int)ceilf((float)(p + 1) * bin) + s;
}

// A pooled rectangle: start, unclipped reach [start, start + ceil(P * bin)), bin sizes.
struct BinRect {
  int x0, y0, xe, ye;
  float bw, bh;
  BinRect() = default;
  __device__ __forceinline__ BinRect(int x0_, int y0_, int x1, int y1, int PH, int PW)
      : x0(x0_), y0(y0_), bw(bin_size(x0_, x1, PW)), bh(bin_size(y0_, y1, PH)) {
    xe = bin_hi(PW - 1, bw, x0);
    ye = bin_hi(PH - 1, bh, y0);
  }
  __device__ __forceinline__ bool reaches(int h, int w) const { return h >= y0 && h < ye && w >= x0 && w < xe; }
};
static_assert(sizeof(BinRect) == 24, "BinRect is six words");

// f(ph, pw) for the bins of `q` that hold cell (h, w): ph outer, pw inner.  (None does unless q.reaches(h, w): the
// gathers ask that first.)
template <class F>
__device__ __forceinline__ void for_bins_holding(const BinRect& q, int h, int w, int PH, int PW, F&& f) {
  for (int ph = 0; ph < PH; ++ph) {
    if (h < bin_lo(ph, q.bh, q.y0) || h >= bin_hi(ph, q.bh, q.y0)) continue;
    for (int pw = 0; pw < PW; ++pw) {
      if (w < bin_lo(pw, q.bw, q.x0) || w >= bin_hi(pw, q.bw, q.x0)) continue;
      f(ph, pw);
    }
  }
}

template <int VEC> struct VecT;
template <> struct VecT<4> { using T = float4; };
template <> struct VecT<1> { using T = float; };

__device__ __forceinline__ float comp(const float4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
__device__ __forceinline__ float comp(const float& v, int) { return v; }
__device__ __forceinline__ void set_comp(float4& v, int k, float x) {
  if (k == 0) v.x = x; else if (k == 1) v.y = x; else if (k == 2) v.z = x; else v.w = x;
}
__device__ __forceinline__ void set_comp(float& v, int, float x) { v = x; }

// The strict '>' of both contracts: the first cell holding the maximum wins.
__device__ __forceinline__ void update_max(float x, int idx, float& m, int& a) {
  if (x > m) { m = x; a = idx; }
}
template <int VEC, class V>
__device__ __forceinline__ void update_max(const V& v, int idx, V& m, int (&a)[VEC]) {
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    const float x = comp(v, k);
    if (x > comp(m, k)) { set_comp(m, k, x); a[k] = idx; }
  }
}

// The backward gather's addition: the gradients of pooled row `row` (VEC channels at c) whose argmax names cell idx.
template <int VEC>
__device__ __forceinline__ void gather_add(float (&acc)[VEC], const float* __restrict__ grad,
                                           const int* __restrict__ argmax, size_t row, int C, int c, int idx) {
  const size_t o = row * C + c;
#pragma unroll
  for (int k = 0; k < VEC; ++k)
    if (argmax[o + k] == idx) acc[k] += grad[o + k];
}

// Host side of a forward entry point: checks, the 16-byte-per-lane choice, grids, launch check.  `op` names the operator
// in the messages; K4 / K1 are its channels-last kernels (one wavefront per (roi, bin row)), KN its NCHW kernel.
template <auto K4, auto K1, auto KN>
int pool_forward(const char* op, const float* input, const float* rois, float* output, int32_t* argmax, int B, int C,
                 int H, int W, int R, float spatial_scale, int pooled_h, int pooled_w, int layout, void* stream) {
  JTSM_REQUIRE(B >= 0 && C >= 0 && H >= 0 && W >= 0 && R >= 0 && pooled_h > 0 && pooled_w > 0, "%s: negative size", op);
  JTSM_REQUIRE(layout == JTSM_NCHW || layout == JTSM_NHWC, "%s: unknown layout %d", op, layout);
  if ((long)R * C == 0) return JTSM_OK;
  JTSM_REQUIRE(input && rois && output && argmax, "%s: null pointer", op);
  JTSM_REQUIRE(B > 0 && H > 0 && W > 0, "%s: empty feature map", op);
  JTSM_REQUIRE((long)H * W < (1L << 31), "%s: map too large for int32 argmax", op);
  hipStream_t st = as_stream(stream);
  if (layout == JTSM_NHWC) {
    const int blocks = ceil_div((long)R * pooled_h, 4);
    const bool v4 = C % 4 == 0 && ((uintptr_t)input & 15) == 0 && ((uintptr_t)output & 15) == 0;
    const auto kernel = v4 ? K4 : K1;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, input, rois, output, argmax, B, C, H, W, R, spatial_scale,
                       pooled_h, pooled_w);
  } else {
    const long total = (long)R * C * pooled_h * pooled_w;
    const int blocks = (int)std::min<long>(ceil_div(total, 256), 8192);
    hipLaunchKernelGGL(KN, dim3(blocks), dim3(256), 0, st, input, rois, output, argmax, B, C, H, W, R, spatial_scale,
                       pooled_h, pooled_w);
  }
  const hipError_t e = hipGetLastError();   // (JTSM_CHECK_LAUNCH with the operator's name in front)
  if (e != hipSuccess) return fail(JTSM_ELAUNCH, "%s forward: %s", op, hipGetErrorString(e));
  return JTSM_OK;
}

template <class Reach>
size_t pool_backward_workspace_bytes(int R) { return R > 0 ? (size_t)R * sizeof(Reach) : 16; }

// Host side of a backward entry point.  KR fills one Reach record per roi into the workspace; G4 / G1 are the gathers
// (one wavefront per (image, cell), grid.y over 64*VEC-channel blocks).
template <class Reach, auto KR, auto G4, auto G1>
int pool_backward(const char* op, const float* grad, const float* rois, const int32_t* argmax, float* grad_input,
                  void* workspace, int B, int C, int H, int W, int R, float spatial_scale, int pooled_h, int pooled_w,
                  void* stream) {
  JTSM_REQUIRE(B >= 0 && C >= 0 && H >= 0 && W >= 0 && R >= 0 && pooled_h > 0 && pooled_w > 0,
               "%s backward: negative size", op);
  const long cells = (long)B * H * W;
  if (cells * C == 0) return JTSM_OK;
  JTSM_REQUIRE(grad_input && workspace, "%s backward: null grad_input / workspace", op);
  JTSM_REQUIRE(R == 0 || (grad && rois && argmax), "%s backward: null pointer", op);
  JTSM_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s backward: workspace must be 16-byte aligned", op);
  hipStream_t st = as_stream(stream);
  Reach* reach = reinterpret_cast<Reach*>(workspace);
  if (R > 0)
    hipLaunchKernelGGL(KR, dim3(ceil_div(R, 256)), dim3(256), 0, st, rois, reach, R, H, W, spatial_scale, pooled_h,
                       pooled_w);
  const bool v4 = C % 4 == 0 && ((uintptr_t)grad_input & 15) == 0 && ((uintptr_t)grad & 15) == 0;
  const dim3 grid(ceil_div(cells, 4), ceil_div(C, 64 * (v4 ? 4 : 1)));
  const auto gather = v4 ? G4 : G1;
  hipLaunchKernelGGL(gather, grid, dim3(256), 0, st, grad, argmax, reach, grad_input, B, C, H, W, R, pooled_h, pooled_w);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(JTSM_ELAUNCH, "%s backward: %s", op, hipGetErrorString(e));
  return JTSM_OK;
}

}  // namespace jtsm
