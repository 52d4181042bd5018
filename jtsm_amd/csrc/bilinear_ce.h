// Bilinear xS up-sampling as the kernels that fuse it form it.  For every one of them (the cross-entropies below, the
// Panoptic-DeepLab regression losses, the keypoint head's and PointRend's x2): the source coordinate rule (lerp_scale)
// and the four-tap blend in ATen's association (bilerp).  For the fused "up-sampling + soft-max cross-entropy" kernels
// (semseg_ops.hip: the mean over the non-ignored pixels; deeplab_loss.hip: the per-pixel loss and the hard-pixel mean):
// one output pixel's log-sum-exp and one source pixel's gradient gather.  One definition each, so that a forward and a
// backward — and the losses among themselves — interpolate the same values to the last bit.
// Everything here is inlined under the INCLUDING file's contraction flag (build.py): bilerp's products and sums fuse
// in semseg_ops.hip and deeplab_loss.hip (contraction on) and round one by one in panoptic_deeplab.hip, keypoint.hip
// and point_rend.hip (-ffp-contract=off), as each file's own copy did.
#pragma once
#include <hip/hip_runtime.h>

namespace jtsm {

// ---- bilinear xS (align_corners = False): src coordinate of dst o is (o + 0.5) / S - 0.5 clamped at 0; taps i0, i1
// with weights l0 = 1 - l1, l1.  x2: inv_scale = 0.5, i.e. o/2 - 0.25 -----------
struct Lerp { int i0, i1; float l0, l1; };
__device__ __forceinline__ Lerp lerp_scale(int o, int n_src, float inv_scale) {
  float s = ((float)o + 0.5f) * inv_scale - 0.5f;
  if (s < 0.f) s = 0.f;
  Lerp r;
  r.i0 = (int)s;
  r.i1 = r.i0 < n_src - 1 ? r.i0 + 1 : r.i0;
  r.l1 = s - (float)r.i0;
  r.l0 = 1.f - r.l1;
  return r;
}

// the four taps (row a.i0: x00, x01; row a.i1: x10, x11) blended in ATen's association
__device__ __forceinline__ float blend(const Lerp& a, const Lerp& b, float x00, float x01, float x10, float x11) {
  return a.l0 * (b.l0 * x00 + b.l1 * x01) + a.l1 * (b.l0 * x10 + b.l1 * x11);
}
// the same read from a map of rows of Ws pixels of ld floats; base: the image's first pixel, at the wanted channel
__device__ __forceinline__ float bilerp(const float* __restrict__ base, int ld, int Ws, const Lerp& a, const Lerp& b) {
  const float x00 = base[((size_t)a.i0 * Ws + b.i0) * ld], x01 = base[((size_t)a.i0 * Ws + b.i1) * ld];
  const float x10 = base[((size_t)a.i1 * Ws + b.i0) * ld], x11 = base[((size_t)a.i1 * Ws + b.i1) * ld];
  return blend(a, b, x00, x01, x10, x11);
}

// l0 * a + l1 * b with the contraction spelled out: the backward forms must round alike
__device__ __forceinline__ float mix2(float l0, float a, float l1, float b) { return __fmaf_rn(l0, a, l1 * b); }

// One output pixel (n, oh, ow) of the forward: its <= 64 logits interpolated from the stride-S map `z` (rows of ldc
// floats, ldc % 4 == 0, C classes) in registers; returns the log-sum-exp and, in `vt`, the logit of class `t` (0 where t
// is no class).
__device__ __forceinline__ float ce_pixel_lse(const float* __restrict__ z, int ldc, int C, int n, int oh, int ow, int Hs,
                                              int Ws, float inv, long t, float& vt) {
  const int nch = ldc >> 2;   // float4 chunks per pixel row (<= 16)
  const Lerp a = lerp_scale(oh, Hs, inv), b = lerp_scale(ow, Ws, inv);
  const float* zn = z + (size_t)n * Hs * Ws * ldc;
  const float4* p00 = reinterpret_cast<const float4*>(zn + ((size_t)a.i0 * Ws + b.i0) * ldc);
  const float4* p01 = reinterpret_cast<const float4*>(zn + ((size_t)a.i0 * Ws + b.i1) * ldc);
  const float4* p10 = reinterpret_cast<const float4*>(zn + ((size_t)a.i1 * Ws + b.i0) * ldc);
  const float4* p11 = reinterpret_cast<const float4*>(zn + ((size_t)a.i1 * Ws + b.i1) * ldc);
  float v[64];
  float mx = -3.0e38f;
  vt = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (j < nch) {
      const float4 v00 = p00[j], v01 = p01[j], v10 = p10[j], v11 = p11[j];
      const float x00[4] = {v00.x, v00.y, v00.z, v00.w}, x01[4] = {v01.x, v01.y, v01.z, v01.w};
      const float x10[4] = {v10.x, v10.y, v10.z, v10.w}, x11[4] = {v11.x, v11.y, v11.z, v11.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 4 * j + e;
        float x = blend(a, b, x00[e], x01[e], x10[e], x11[e]);
        if (c >= C) x = -3.0e38f;
        v[c] = x;
        mx = fmaxf(mx, x);
        vt = (long)c == t ? x : vt;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * j + e] = -3.0e38f;
    }
  }
  float sm = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (j < nch) {
#pragma unroll
      for (int e = 0; e < 4; ++e) sm += __expf(v[4 * j + e] - mx);
    }
  return mx + __logf(sm);
}

// One source pixel (n, h, w), channels c0 .. c0 + 3, of the backward:
//   acc[e] = sum over output pixels o touching (h, w) of weight(o -> (h, w)) * coef(o) * (softmax_o[c0 + e] - [c0 + e == t_o])
// A gather (no atomics, deterministic).  For one output column the three source rows h-1, h, h+1 are interpolated along
// x once and reused by all of that column's output rows.  COEF: `coef` holds one factor per output pixel (0: the pixel
// is skipped); otherwise the factor is 1.  Ignored pixels are skipped either way.
template <bool COEF>
__device__ __forceinline__ void ce_gather_source(const float* __restrict__ z, int ldc, int C,
                                                 const long* __restrict__ target, const float* __restrict__ lse,
                                                 const float* __restrict__ coef, int n, int h, int w, int c0, int Hs,
                                                 int Ws, int S, float inv, long ignore, float (&acc)[4]) {
  const int H = Hs * S, W = Ws * S;
  const float* zn = z + (size_t)n * Hs * Ws * ldc + c0;
  const int hm = max(h - 1, 0), hp = min(h + 1, Hs - 1);
  acc[0] = acc[1] = acc[2] = acc[3] = 0.f;
  // rows / columns of the output that can put weight on (h, w): exact for even S, one spare each side for odd S
  const int oh0 = max(S * h - (S + 1) / 2, 0), oh1 = min(S * h + S + (S + 1) / 2, H);
  const int ow0 = max(S * w - (S + 1) / 2, 0), ow1 = min(S * w + S + (S + 1) / 2, W);
  for (int ow = ow0; ow < ow1; ++ow) {
    const Lerp b = lerp_scale(ow, Ws, inv);
    const float wx = (b.i0 == w ? b.l0 : 0.f) + (b.i1 == w ? b.l1 : 0.f);
    if (wx == 0.f) continue;
    float r[3][4];   // x-interpolated logits of source rows h-1, h, h+1 at this output column
    const int rows[3] = {hm, h, hp};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float4 u0 = *reinterpret_cast<const float4*>(zn + ((size_t)rows[i] * Ws + b.i0) * ldc);
      const float4 u1 = *reinterpret_cast<const float4*>(zn + ((size_t)rows[i] * Ws + b.i1) * ldc);
      r[i][0] = mix2(b.l0, u0.x, b.l1, u1.x); r[i][1] = mix2(b.l0, u0.y, b.l1, u1.y);
      r[i][2] = mix2(b.l0, u0.z, b.l1, u1.z); r[i][3] = mix2(b.l0, u0.w, b.l1, u1.w);
    }
    for (int oh = oh0; oh < oh1; ++oh) {
      const Lerp a = lerp_scale(oh, Hs, inv);
      const float wy = (a.i0 == h ? a.l0 : 0.f) + (a.i1 == h ? a.l1 : 0.f);
      if (wy == 0.f) continue;
      const long o = ((long)n * H + oh) * W + ow;
      const long t = target[o];
      if (t == ignore) continue;
      float wgt = wy * wx;
      if (COEF) {
        const float k = coef[o];
        if (k == 0.f) continue;
        wgt *= k;
      }
      const float l = lse[o];
      const bool lo0 = a.i0 < h, hi0 = a.i0 > h, lo1 = a.i1 < h, hi1 = a.i1 > h;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t0 = lo0 ? r[0][e] : (hi0 ? r[2][e] : r[1][e]);
        const float t1 = lo1 ? r[0][e] : (hi1 ? r[2][e] : r[1][e]);
        const float v = mix2(a.l0, t0, a.l1, t1);
        const float pr = c0 + e < C ? __expf(v - l) : 0.f;
        acc[e] = __fmaf_rn(wgt, pr - ((long)(c0 + e) == t ? 1.f : 0.f), acc[e]);
      }
    }
  }
}

}  // namespace jtsm
