// Deformable convolution v1 / v2 (detectron2/layers/csrc/deformable/deform_conv_cuda_kernel.cu) as three kernels
// around the existing contraction: the sampled columns, the offset / mask gradient and the input gradient.
// DESIGN.md §4j.  Built with -ffp-contract=off: the sampling arithmetic is the reference's, product by product.
//
// Layouts (channels-last throughout): x (N, H, W, C); offset (N, Ho, Wo, G * 2 * K) and mask (N, Ho, Wo, G * K) with
// K = kh * kw taps, channel 2k = dy and 2k + 1 = dx of tap k inside a deformable group; cols / dcols
// (N * Ho * Wo, K, C), tap-major and channel-minor — the order of an (O, kh, kw, C) weight's rows.
//
// A UNIT is one (pixel, tap, group): u = (pixel * K + tap) * G + group.  2^lpu_shift lanes (LPU: the power of two at or
// above Cg / 4, at most 64) share a unit and run along its Cg = C / G channels four at a time, so the offsets and the
// bilinear weights are computed once per unit and every access to x / cols is a 16-byte piece of one NHWC row.
#include "common.h"
#include "sorted_segments.h"
#include "workspace.h"

namespace jtsm {
namespace {

struct DeformGeo {
  int N, H, W, C, G, Cg, kh, kw, K, stride, pad, dil, Ho, Wo;
  long pixels, units;   // N * Ho * Wo, pixels * K * G
};

// The sampling point of a unit and its bilinear frame (deformable_im2col_bilinear / dmcn_im2col_bilinear).
struct Sample {
  float h, w, m;
  int hl, wl;
  bool in;              // h > -1 && w > -1 && h < H && w < W
  long pixel;
  int tap, g, n;
};

__device__ __forceinline__ Sample locate(const DeformGeo& q, long u, const float* __restrict__ offset,
                                         const float* __restrict__ mask) {
  Sample s;
  s.g = (int)(u % q.G);
  const long pk = u / q.G;
  s.tap = (int)(pk % q.K);
  s.pixel = pk / q.K;
  const int ox = (int)(s.pixel % q.Wo), oy = (int)((s.pixel / q.Wo) % q.Ho);
  s.n = (int)(s.pixel / ((long)q.Wo * q.Ho));
  const int i = s.tap / q.kw, j = s.tap % q.kw;
  const float* o2 = offset + (s.pixel * q.G + s.g) * (2 * q.K) + 2 * s.tap;
  s.h = (float)(oy * q.stride - q.pad + i * q.dil) + o2[0];
  s.w = (float)(ox * q.stride - q.pad + j * q.dil) + o2[1];
  s.m = mask ? mask[(s.pixel * q.G + s.g) * q.K + s.tap] : 1.f;
  s.in = s.h > -1.f && s.w > -1.f && s.h < (float)q.H && s.w < (float)q.W;
  s.hl = s.in ? (int)floorf(s.h) : 0;
  s.wl = s.in ? (int)floorf(s.w) : 0;
  return s;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// The four corners' values of one 4-channel piece; a corner outside the map (or a sample outside) reads as zero.
struct Corners { float4 v1, v2, v3, v4; };
__device__ __forceinline__ Corners corners(const DeformGeo& q, const Sample& s, const float* __restrict__ xg, int c) {
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  Corners r{z, z, z, z};
  if (!s.in) return r;
  const int hh = s.hl + 1, wh = s.wl + 1;
  const long row = (long)q.W * q.C;
  if (s.hl >= 0 && s.wl >= 0) r.v1 = ld4(xg + s.hl * row + (long)s.wl * q.C + c);
  if (s.hl >= 0 && wh <= q.W - 1) r.v2 = ld4(xg + s.hl * row + (long)wh * q.C + c);
  if (hh <= q.H - 1 && s.wl >= 0) r.v3 = ld4(xg + hh * row + (long)s.wl * q.C + c);
  if (hh <= q.H - 1 && wh <= q.W - 1) r.v4 = ld4(xg + hh * row + (long)wh * q.C + c);
  return r;
}

// ---- (a) columns --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void deform_columns_kernel(const float* __restrict__ x, const float* __restrict__ offset,
                                                             const float* __restrict__ mask, float* __restrict__ cols,
                                                             DeformGeo q, int lpu_shift) {
  const long u = (long)blockIdx.x * (256 >> lpu_shift) + (threadIdx.x >> lpu_shift);
  const int sub = threadIdx.x & ((1 << lpu_shift) - 1);
  if (u >= q.units) return;
  const Sample s = locate(q, u, offset, mask);
  const float lh = s.h - (float)s.hl, lw = s.w - (float)s.wl;
  const float hh = 1.f - lh, hw = 1.f - lw;
  const float w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
  const float* xg = x + (long)s.n * q.H * q.W * q.C + s.g * q.Cg;
  float* out = cols + (s.pixel * q.K + s.tap) * q.C + s.g * q.Cg;
  for (int c = sub * 4; c < q.Cg; c += 4 << lpu_shift) {
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s.in) {
      const Corners v = corners(q, s, xg, c);
      r.x = (w1 * v.v1.x + w2 * v.v2.x + w3 * v.v3.x + w4 * v.v4.x) * s.m;
      r.y = (w1 * v.v1.y + w2 * v.v2.y + w3 * v.v3.y + w4 * v.v4.y) * s.m;
      r.z = (w1 * v.v1.z + w2 * v.v2.z + w3 * v.v3.z + w4 * v.v4.z) * s.m;
      r.w = (w1 * v.v1.w + w2 * v.v2.w + w3 * v.v3.w + w4 * v.v4.w) * s.m;
    }
    *reinterpret_cast<float4*>(out + c) = r;
  }
}

// ---- (b) offset and mask gradient -----------------------------------------------------------------------------------
// get_coordinate_weight / dmcn_get_coordinate_weight per channel, times dcols (and the mask), summed over the group's
// channels: each lane over its pieces in order, then a butterfly over the unit's lanes — one fixed shape, no atomics.
__global__ __launch_bounds__(256) void deform_offset_mask_grad_kernel(
    const float* __restrict__ dcols, const float* __restrict__ x, const float* __restrict__ offset,
    const float* __restrict__ mask, float* __restrict__ d_offset, float* __restrict__ d_mask, DeformGeo q, int lpu_shift) {
  const long u = (long)blockIdx.x * (256 >> lpu_shift) + (threadIdx.x >> lpu_shift);
  const int sub = threadIdx.x & ((1 << lpu_shift) - 1);
  const bool live = u < q.units;
  float ay = 0.f, ax = 0.f, am = 0.f;
  Sample s;
  if (live) {
    s = locate(q, u, offset, mask);
    if (s.in) {
      const float lh = s.h - (float)s.hl, lw = s.w - (float)s.wl;
      const float hh = 1.f - lh, hw = 1.f - lw;
      const float w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
      const float gh = (float)(s.hl + 1) - s.h, gw = (float)(s.wl + 1) - s.w;   // (low + 1 - argmax), (argmax - low) = lh / lw
      const float* xg = x + (long)s.n * q.H * q.W * q.C + s.g * q.Cg;
      const float* dc = dcols + (s.pixel * q.K + s.tap) * q.C + s.g * q.Cg;
      for (int c = sub * 4; c < q.Cg; c += 4 << lpu_shift) {
        const Corners v = corners(q, s, xg, c);
        const float4 d = ld4(dc + c);
#define JTSM_DEFORM_TERM(f)                                                                        \
        {                                                                                          \
          float wy = 0.f, wx = 0.f;                                                                \
          wy += -1.f * gw * v.v1.f; wy += -1.f * lw * v.v2.f; wy += gw * v.v3.f; wy += lw * v.v4.f; \
          wx += -1.f * gh * v.v1.f; wx += gh * v.v2.f; wx += -1.f * lh * v.v3.f; wx += lh * v.v4.f; \
          ay += wy * d.f * s.m;                                                                    \
          ax += wx * d.f * s.m;                                                                    \
          am += d.f * (w1 * v.v1.f + w2 * v.v2.f + w3 * v.v3.f + w4 * v.v4.f);                     \
        }
        JTSM_DEFORM_TERM(x) JTSM_DEFORM_TERM(y) JTSM_DEFORM_TERM(z) JTSM_DEFORM_TERM(w)
#undef JTSM_DEFORM_TERM
      }
    }
  }
  for (int o = (1 << lpu_shift) >> 1; o > 0; o >>= 1) {   // the unit's lanes are 2^lpu_shift aligned neighbours
    ay += __shfl_xor(ay, o);
    ax += __shfl_xor(ax, o);
    am += __shfl_xor(am, o);
  }
  if (live && sub == 0) {
    float* o2 = d_offset + (s.pixel * q.G + s.g) * (2 * q.K) + 2 * s.tap;
    o2[0] = ay;
    o2[1] = ax;
    if (d_mask) d_mask[(s.pixel * q.G + s.g) * q.K + s.tap] = am;
  }
}

// ---- (c) input gradient: keys, sort, walk ---------------------------------------------------------------------------
// One entry per (unit, corner): e = 4 u + corner.  key = destination << ebits | e with destination ((n H + y) W + x) G + g,
// or D (the sentinel class) for a corner outside the map, a sample outside (-1, H) x (-1, W) or a zero weight; the
// sort's value is the bits of get_gradient_weight(...) * mask.
__global__ __launch_bounds__(256) void deform_input_keys_kernel(const float* __restrict__ offset,
                                                                const float* __restrict__ mask, DeformGeo q, long E,
                                                                long D, int ebits, u64* __restrict__ keys,
                                                                int* __restrict__ vals) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const int corner = (int)(e & 3);
  const Sample s = locate(q, e >> 2, offset, mask);
  const int y = s.hl + (corner >> 1), xx = s.wl + (corner & 1);
  long dest = D;
  float wm = 0.f;
  if (s.in && y >= 0 && y < q.H && xx >= 0 && xx < q.W) {
    const float wy = (corner >> 1) ? (s.h + 1.f) - (float)y : (float)(y + 1) - s.h;
    const float wx = (corner & 1) ? (s.w + 1.f) - (float)xx : (float)(xx + 1) - s.w;
    wm = wy * wx * s.m;
    if (wm != 0.f) dest = (((long)s.n * q.H + y) * q.W + xx) * q.G + s.g;
  }
  keys[e] = ((u64)dest << ebits) | (u64)e;
  vals[e] = __float_as_int(wm);
}

// One workgroup per destination (n, y, x, g): its list is start[d] .. start[d + 1] of the sorted entries, ascending in
// e.  The 256 / LPU slices of the workgroup take the list's entries round-robin, lanes along the group's channels; the
// slices' sums meet in LDS by a halving tree.  Every element of dx is written (an empty list writes zeros).
__global__ __launch_bounds__(256) void deform_input_walk_kernel(const float* __restrict__ dcols,
                                                                const u64* __restrict__ keys,
                                                                const int* __restrict__ vals,
                                                                const int* __restrict__ start, DeformGeo q, int ebits,
                                                                int lpu_shift, float* __restrict__ dx) {
  __shared__ float4 part[256];
  const long d = blockIdx.x;
  const int g = (int)(d % q.G);
  const long pix = d / q.G;
  const int lpu = 1 << lpu_shift, slices = 256 >> lpu_shift;
  const int sub = threadIdx.x & (lpu - 1), sl = threadIdx.x >> lpu_shift;
  const int beg = start[d], end = start[d + 1];
  const u64 emask = ((u64)1 << ebits) - 1;
  float* out = dx + pix * q.C + g * q.Cg;
  for (int cbase = 0; cbase < q.Cg; cbase += 4 * lpu) {
    const int c = cbase + sub * 4;
    const bool active = c < q.Cg;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = beg + sl; j < end; j += slices) {
      const long unit = (long)((keys[j] & emask) >> 2);
      const float wm = __int_as_float(vals[j]);
      if (active) {
        const float4 v = ld4(dcols + (unit / q.G) * q.C + g * q.Cg + c);
        acc.x += wm * v.x; acc.y += wm * v.y; acc.z += wm * v.z; acc.w += wm * v.w;
      }
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int o = slices >> 1; o > 0; o >>= 1) {
      if (sl < o) {
        const float4 b = part[threadIdx.x + (o << lpu_shift)];
        float4 a = part[threadIdx.x];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        part[threadIdx.x] = a;
      }
      __syncthreads();
    }
    if (sl == 0 && active) *reinterpret_cast<float4*>(out + c) = part[threadIdx.x];
    __syncthreads();
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------
int make_geo(DeformGeo& q, const char* who, int N, int H, int W, int C, int G, int kh, int kw, int stride, int pad,
             int dil) {
  JTSM_REQUIRE(N >= 0 && H > 0 && W > 0 && C > 0 && G > 0 && kh > 0 && kw > 0 && stride > 0 && pad >= 0 && dil > 0,
               "%s: bad sizes N=%d H=%d W=%d C=%d G=%d kernel %dx%d stride=%d pad=%d dil=%d", who, N, H, W, C, G, kh, kw,
               stride, pad, dil);
  JTSM_REQUIRE(C % G == 0 && (C / G) % 4 == 0, "%s: C / deformable_groups must be a multiple of 4 (C=%d, G=%d)", who, C, G);
  q.N = N; q.H = H; q.W = W; q.C = C; q.G = G; q.Cg = C / G; q.kh = kh; q.kw = kw; q.K = kh * kw;
  q.stride = stride; q.pad = pad; q.dil = dil;
  q.Ho = (H + 2 * pad - dil * (kh - 1) - 1) / stride + 1;
  q.Wo = (W + 2 * pad - dil * (kw - 1) - 1) / stride + 1;
  if (H + 2 * pad - dil * (kh - 1) - 1 < 0) q.Ho = 0;
  if (W + 2 * pad - dil * (kw - 1) - 1 < 0) q.Wo = 0;
  q.pixels = (long)N * q.Ho * q.Wo;
  q.units = q.pixels * q.K * G;
  JTSM_REQUIRE(q.units * 4 <= 2147483647L && (long)N * H * W * G < 2147483647L,
               "%s: %ld samples x 4 corners / %ld destinations do not fit 31 bits (loop over groups of images)", who,
               q.units, (long)N * H * W * G);
  return JTSM_OK;
}

int lanes_shift(const DeformGeo& q) {   // LPU = 2^shift lanes per unit
  int s = 0;
  while (s < 6 && (4 << s) < q.Cg) ++s;
  return s;
}

struct InputGradWs {
  long E, D;
  int ebits, dbits;
  u64 *key_a, *key_b;
  int *val_a, *val_b, *start;
  size_t cub_bytes;
  char* cub;
};

InputGradWs carve(Arena& a, const DeformGeo& q) {
  InputGradWs w;
  w.E = q.units * 4;
  w.D = (long)q.N * q.H * q.W * q.G;
  w.ebits = bits_for(w.E > 0 ? w.E - 1 : 0);
  w.dbits = bits_for(w.D);
  w.key_a = a.take<u64>(w.E);
  w.key_b = a.take<u64>(w.E);
  w.val_a = a.take<int>(w.E);
  w.val_b = a.take<int>(w.E);
  w.start = a.take<int>(w.D + 2);
  w.cub_bytes = w.E > 0 ? sort_pairs_temp_bytes((int)w.E) : 0;
  w.cub = a.take<char>(w.cub_bytes);
  return w;
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" {

int jtsm_deform_columns_f32(const float* x, const float* offset, const float* mask, float* cols, int N, int H, int W,
                            int C, int G, int kh, int kw, int stride, int pad, int dil, void* stream) {
  DeformGeo q;
  if (int rc = make_geo(q, "deform_columns", N, H, W, C, G, kh, kw, stride, pad, dil)) return rc;
  if (q.units == 0) return JTSM_OK;
  JTSM_REQUIRE(x && offset && cols, "deform_columns: null pointer");
  const int sh = lanes_shift(q);
  hipLaunchKernelGGL(deform_columns_kernel, dim3(ceil_div(q.units, 256 >> sh)), dim3(256), 0, as_stream(stream), x,
                     offset, mask, cols, q, sh);
  JTSM_CHECK_LAUNCH("deform_columns");
  return JTSM_OK;
}

int jtsm_deform_offset_mask_grad_f32(const float* dcols, const float* x, const float* offset, const float* mask,
                                     float* d_offset, float* d_mask, int N, int H, int W, int C, int G, int kh, int kw,
                                     int stride, int pad, int dil, void* stream) {
  DeformGeo q;
  if (int rc = make_geo(q, "deform_offset_mask_grad", N, H, W, C, G, kh, kw, stride, pad, dil)) return rc;
  if (q.units == 0) return JTSM_OK;
  JTSM_REQUIRE(dcols && x && offset && d_offset, "deform_offset_mask_grad: null pointer");
  JTSM_REQUIRE(!d_mask || mask, "deform_offset_mask_grad: d_mask without a mask");
  const int sh = lanes_shift(q);
  hipLaunchKernelGGL(deform_offset_mask_grad_kernel, dim3(ceil_div(q.units, 256 >> sh)), dim3(256), 0,
                     as_stream(stream), dcols, x, offset, mask, d_offset, d_mask, q, sh);
  JTSM_CHECK_LAUNCH("deform_offset_mask_grad");
  return JTSM_OK;
}

size_t jtsm_deform_input_grad_workspace_bytes(int N, int H, int W, int G, int kh, int kw, int stride, int pad, int dil) {
  DeformGeo q;
  if (make_geo(q, "deform_input_grad_workspace_bytes", N, H, W, 4 * G, G, kh, kw, stride, pad, dil)) return 0;
  Arena a{nullptr};
  carve(a, q);
  return a.off;
}

int jtsm_deform_input_grad_f32(const float* dcols, const float* offset, const float* mask, float* dx, int N, int H,
                               int W, int C, int G, int kh, int kw, int stride, int pad, int dil, void* workspace,
                               size_t workspace_bytes, void* stream) {
  DeformGeo q;
  if (int rc = make_geo(q, "deform_input_grad", N, H, W, C, G, kh, kw, stride, pad, dil)) return rc;
  if (N == 0) return JTSM_OK;
  JTSM_REQUIRE(dx, "deform_input_grad: null pointer");
  hipStream_t st = as_stream(stream);
  if (q.units == 0) {   // no output pixel: nothing reaches x
    JTSM_CHECK_HIP(hipMemsetAsync(dx, 0, sizeof(float) * (size_t)N * H * W * C, st));
    return JTSM_OK;
  }
  JTSM_REQUIRE(dcols && offset, "deform_input_grad: null pointer");
  Arena arena{static_cast<char*>(workspace)};
  const InputGradWs w = carve(arena, q);
  JTSM_REQUIRE(workspace && workspace_bytes >= arena.off && ((size_t)workspace & 255) == 0,
               "deform_input_grad: workspace of %zu bytes (256-byte aligned) needed", arena.off);
  JTSM_REQUIRE(w.ebits + w.dbits <= 64, "deform_input_grad: key of %d + %d bits", w.dbits, w.ebits);
  hipLaunchKernelGGL(deform_input_keys_kernel, dim3(ceil_div(w.E, 256)), dim3(256), 0, st, offset, mask, q, w.E, w.D,
                     w.ebits, w.key_a, w.val_a);
  JTSM_CHECK_LAUNCH("deform input keys");
  // stable, and over the destination bits only: inside a destination the entries keep their emission order, e ascending
  size_t cub_bytes = w.cub_bytes;
  JTSM_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(w.cub, cub_bytes, w.key_a, w.key_b, w.val_a, w.val_b, (int)w.E,
                                                    w.ebits, w.ebits + w.dbits, st));
  hipLaunchKernelGGL(segment_starts_kernel, dim3(ceil_div(w.D + 1, 64)), dim3(64), 0, st, w.key_b, (int)w.E, (int)w.D,
                     w.ebits, w.start);
  JTSM_CHECK_LAUNCH("deform input segments");
  hipLaunchKernelGGL(deform_input_walk_kernel, dim3((unsigned)w.D), dim3(256), 0, st, dcols, w.key_b, w.val_b, w.start,
                     q, w.ebits, lanes_shift(q), dx);
  JTSM_CHECK_LAUNCH("deform input walk");
  return JTSM_OK;
}

}  // extern "C"
