// Box arithmetic that decides integers (which box wins, which is suppressed), shared by the kernels that must agree
// on it bit for bit: evaluated un-contracted, in the reference's operation order.
#pragma once
#include <hip/hip_runtime.h>

namespace jtsm {

__device__ __forceinline__ void decode_box(const float* __restrict__ p, const float* __restrict__ d, float* out) {
#pragma clang fp contract(off)
  // Box2BoxTransform(10,10,5,5).apply_deltas for one (box, class) pair
  const float w = p[2] - p[0], h = p[3] - p[1];
  const float cx = p[0] + 0.5f * w, cy = p[1] + 0.5f * h;
  const float dx = d[0] / 10.f, dy = d[1] / 10.f;
  const float kClamp = 4.135166556742356f;  // log(1000/16)
  const float dw = fminf(d[2] / 5.f, kClamp), dh = fminf(d[3] / 5.f, kClamp);
  const float pcx = dx * w + cx, pcy = dy * h + cy;
  const float pw = expf(dw) * w, ph = expf(dh) * h;
  out[0] = pcx - 0.5f * pw;
  out[1] = pcy - 0.5f * ph;
  out[2] = pcx + 0.5f * pw;
  out[3] = pcy + 0.5f * ph;
}

// detectron2's pairwise_iou in float32, every step rounded on its own (PCL's graph and cluster assignment, C-MIL's
// ROIMerge and ROILabel: none of them builds the R x R matrix the reference reads these values from)
__device__ __forceinline__ float box_iou(const float4 a, const float4 b) {
#pragma clang fp contract(off)
  const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f);
  const float h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
  const float inter = w * h;
  const float aa = (a.z - a.x) * (a.w - a.y), ab = (b.z - b.x) * (b.w - b.y);
  return inter > 0.f ? inter / (aa + ab - inter) : 0.f;
}

// Row r of a (n, 4) box array: load_box in one 16-byte load, for entry points that require the alignment; box_at in
// four loads, for those that do not promise it.
__device__ __forceinline__ float4 load_box(const float* __restrict__ boxes, long r) {
  return *reinterpret_cast<const float4*>(boxes + r * 4);
}
__device__ __forceinline__ float4 box_at(const float* __restrict__ boxes, long r) {
  const float* __restrict__ p = boxes + r * 4;
  return make_float4(p[0], p[1], p[2], p[3]);
}

// torchvision's nms IoU test (ops/csrc/cuda/nms_cuda.cu devIoU @0.8.1; the CPU kernel computes the same expression)
__device__ __forceinline__ bool iou_above(const float4& a, const float4& b, float thr) {
#pragma clang fp contract(off)
  const float left = fmaxf(a.x, b.x), right = fminf(a.z, b.z);
  const float top = fmaxf(a.y, b.y), bottom = fminf(a.w, b.w);
  const float width = fmaxf(right - left, 0.f), height = fmaxf(bottom - top, 0.f);
  const float inter = width * height;
  const float sa = (a.z - a.x) * (a.w - a.y);
  const float sb = (b.z - b.x) * (b.w - b.y);
  return (inter / (sa + sb - inter)) > thr;
}

}  // namespace jtsm
