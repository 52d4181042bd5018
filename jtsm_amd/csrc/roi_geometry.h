// Device-side ROI sampling geometry shared by ROIAlign / ROIAlignRotated kernels and the
// sample-table dump.  Behaviour contract: SURVEY.md Appendix A.1/A.2, i.e. the arithmetic of
//   detectron2/layers/csrc/ROIAlign/ROIAlign_cpu.cpp:20-114,134-169   (axis-aligned)
//   detectron2/layers/csrc/ROIAlignRotated/ROIAlignRotated_cpu.cpp:27-129,218-261 (rotated)
// The integer results (grid size, y_low/x_low/..., validity) must equal the CPU path's bit for
// bit, so every floating-point step here is individually rounded: FMA contraction is switched
// off for this header (hipcc contracts by default; the x86-64 reference build has no FMA).
#pragma once
#include <hip/hip_runtime.h>

namespace jtsm {

#pragma clang fp contract(off)

template <typename T>
struct Tap {
  int pos[4];  // flat y*W+x of the four neighbours; pos[0] == -1 marks "out of range"
  T w[4];
};

template <typename T>
struct RoiGeom {
  int b;
  T y0, x0, bh, bw;
  int gh, gw;
  T cy, cx, cs, sn;
};

template <typename T> __device__ __forceinline__ T ceil_t(T v);
template <> __device__ __forceinline__ float ceil_t<float>(float v) { return ceilf(v); }
template <> __device__ __forceinline__ double ceil_t<double>(double v) { return ceil(v); }

// Axis-aligned box (x0,y0,x1,y1).  Negative extents in aligned mode give an empty grid
// (the CUDA reference does the same; only its CPU path asserts, ROIAlign_cpu.cpp:149-152).
template <typename T>
__device__ __forceinline__ RoiGeom<T> geom_box(const T* __restrict__ roi, T scale, int PH,
                                               int PW, int sampling_ratio, bool aligned) {
#pragma clang fp contract(off)
  RoiGeom<T> g;
  g.b = (int)roi[0];
  const T off = aligned ? (T)0.5 : (T)0.0;
  const T sx = roi[1] * scale - off, sy = roi[2] * scale - off;
  const T ex = roi[3] * scale - off, ey = roi[4] * scale - off;
  T rw = ex - sx, rh = ey - sy;
  if (!aligned) {
    rw = rw < (T)1 ? (T)1 : rw;
    rh = rh < (T)1 ? (T)1 : rh;
  }
  g.y0 = sy;
  g.x0 = sx;
  g.bh = rh / (T)PH;
  g.bw = rw / (T)PW;
  g.gh = sampling_ratio > 0 ? sampling_ratio : (int)ceil_t<T>(rh / (T)PH);
  g.gw = sampling_ratio > 0 ? sampling_ratio : (int)ceil_t<T>(rw / (T)PW);
  g.cy = g.cx = (T)0;
  g.cs = (T)1;
  g.sn = (T)0;
  return g;
}

// Rotated box (cx,cy,w,h,deg).  The reference evaluates the angle in double and calls the
// double cos/sin, rounding the results to T (ROIAlignRotated_cpu.cpp:232-234).
template <typename T>
__device__ __forceinline__ RoiGeom<T> geom_rbox(const T* __restrict__ roi, T scale, int PH,
                                                int PW, int sampling_ratio) {
#pragma clang fp contract(off)
  RoiGeom<T> g;
  g.b = (int)roi[0];
  g.cx = roi[1] * scale - (T)0.5;
  g.cy = roi[2] * scale - (T)0.5;
  const T rw = roi[3] * scale, rh = roi[4] * scale;
  const T theta = (T)((double)roi[5] * 3.14159265358979323846 / 180.0);
  g.cs = (T)cos((double)theta);
  g.sn = (T)sin((double)theta);
  g.bh = rh / (T)PH;
  g.bw = rw / (T)PW;
  g.gh = sampling_ratio > 0 ? sampling_ratio : (int)ceil_t<T>(rh / (T)PH);
  g.gw = sampling_ratio > 0 ? sampling_ratio : (int)ceil_t<T>(rw / (T)PW);
  g.y0 = (T)(-(double)rh / 2.0);
  g.x0 = (T)(-(double)rw / 2.0);
  return g;
}

// One axis of a bilinear sample on a line of n cells.  A coordinate outside [-1, n] drops the whole sample; inside, the
// two cells and their weights: clamped at 0, the last line folded onto itself.  STRICT selects the rotated variant's
// "y < 0" clamp test.  The one statement of the rule: make_tap takes two of these, the gather form of the backward
// (roi_align.hip, align_bwd_gather) stages its per-axis weights from the same pair.  The range test stays a function
// of its own, called BEFORE the clamp: folded into axis_tap as a sentinel it lengthened every kernel.
template <typename T> __device__ __forceinline__ bool axis_outside(int n, T y) { return y < (T)-1.0 || y > (T)n; }
template <typename T> struct AxisTap { int lo, hi; T w_lo, w_hi; };
template <typename T, bool STRICT>
__device__ __forceinline__ AxisTap<T> axis_tap(int n, T y) {
#pragma clang fp contract(off)
  AxisTap<T> a;
  if (STRICT) { if (y < (T)0) y = (T)0; } else { if (y <= (T)0) y = (T)0; }
  a.lo = (int)y;
  if (a.lo >= n - 1) { a.hi = a.lo = n - 1; y = (T)a.lo; } else { a.hi = a.lo + 1; }
  a.w_hi = y - (T)a.lo;
  a.w_lo = (T)1 - a.w_hi;
  return a;
}

// One bilinear sample: both axes in range, then four positions and four products.
template <typename T, bool STRICT>
__device__ __forceinline__ Tap<T> make_tap(int H, int W, T y, T x) {
#pragma clang fp contract(off)
  Tap<T> t;
  if (axis_outside(H, y) || axis_outside(W, x)) {
    t.pos[0] = t.pos[1] = t.pos[2] = t.pos[3] = -1;
    t.w[0] = t.w[1] = t.w[2] = t.w[3] = (T)0;
    return t;
  }
  const AxisTap<T> ay = axis_tap<T, STRICT>(H, y), ax = axis_tap<T, STRICT>(W, x);
  t.pos[0] = ay.lo * W + ax.lo;
  t.pos[1] = ay.lo * W + ax.hi;
  t.pos[2] = ay.hi * W + ax.lo;
  t.pos[3] = ay.hi * W + ax.hi;
  t.w[0] = ay.w_lo * ax.w_lo;
  t.w[1] = ay.w_lo * ax.w_hi;
  t.w[2] = ay.w_hi * ax.w_lo;
  t.w[3] = ay.w_hi * ax.w_hi;
  return t;
}

template <typename T, bool ROT>
__device__ __forceinline__ Tap<T> sample_tap(const RoiGeom<T>& g, int H, int W, int ph, int pw,
                                             int iy, int ix) {
#pragma clang fp contract(off)
  // (T)(iy + .5f): the reference forms the half-offset in float first, also for double.
  const T yy = g.y0 + (T)ph * g.bh + (T)((float)iy + .5f) * g.bh / (T)g.gh;
  const T xx = g.x0 + (T)pw * g.bw + (T)((float)ix + .5f) * g.bw / (T)g.gw;
  if (!ROT) return make_tap<T, false>(H, W, yy, xx);
  const T y = yy * g.cs - xx * g.sn + g.cy;
  const T x = yy * g.sn + xx * g.cs + g.cx;
  return make_tap<T, true>(H, W, y, x);
}

template <typename T, bool ROT>
__device__ __forceinline__ RoiGeom<T> roi_geometry(const T* __restrict__ rois, int n, T scale,
                                                   int PH, int PW, int sampling_ratio,
                                                   bool aligned) {
  return ROT ? geom_rbox<T>(rois + (size_t)n * 6, scale, PH, PW, sampling_ratio)
             : geom_box<T>(rois + (size_t)n * 5, scale, PH, PW, sampling_ratio, aligned);
}

}  // namespace jtsm
