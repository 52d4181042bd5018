// Operand planes: the definition, in code, once.  An fp32 value x stands beside either
//     two bf16 planes   hi = bf16(x),  lo = bf16(x - hi)          (split-bf16: x = hi + lo up to 2^-17 |x|)
//     one fp16 plane    h  = f16(ldexp(x, shift))                  (lo == nullptr everywhere below)
// Every producer writes its plane words through this header and every reader takes them back through it, so the words
// cannot drift from the fp32 value stored beside them (tests/test_hip_planes.py compares each producer word for word).
#pragma once
#include <hip/hip_runtime.h>

namespace jtsm {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
// N = 4 or 8 plane words: 8 or 16 bytes per plane
template <int N> struct PlaneWords;
template <> struct PlaneWords<4> { typedef bf16x4 bf16; typedef f16x4 f16; };
template <> struct PlaneWords<8> { typedef bf16x8 bf16; typedef f16x8 f16; };

// The fp16 plane word of v * 2^shift.  ldexp, not a multiply: a multiply in front of the conversion is folded into
// v_fma_mix{lo,hi}_f16 (v * s + 0) on SOME lanes of an unrolled group, and -0 + 0 is +0 — the plane of a stored -0 then
// depended on the element's position (tests/test_hip_planes.py).
__device__ __forceinline__ _Float16 f16_plane(float v, int shift) { return (_Float16)__builtin_ldexpf(v, shift); }

// The bf16 pair of v.  The residual is that of the STORED value: the subtraction is formed with contraction off, so a
// caller's `v = a * s` is never fused into it (a * s - hi rounds once and gives other bits), whatever flags the
// including file is built with.
__device__ __forceinline__ void split_bf16(float v, __bf16& h, __bf16& l) {
#pragma clang fp contract(off)
  h = (__bf16)v;
  l = (__bf16)(v - (float)h);
}

template <int N>
__device__ __forceinline__ void split_planes(const float (&v)[N], typename PlaneWords<N>::bf16& h,
                                             typename PlaneWords<N>::bf16& l) {
#pragma unroll
  for (int e = 0; e < N; ++e) {
    __bf16 hh, ll;
    split_bf16(v[e], hh, ll);
    h[e] = hh; l[e] = ll;
  }
}
template <int N>
__device__ __forceinline__ typename PlaneWords<N>::f16 f16_planes(const float (&v)[N], int shift) {
  typename PlaneWords<N>::f16 h;
#pragma unroll
  for (int e = 0; e < N; ++e) h[e] = f16_plane(v[e], shift);
  return h;
}

// The writer: plane words of N finished values at element offset o (a multiple of N; 2 N bytes per plane).  lo ==
// nullptr: ONE fp16 plane of v * 2^shift in `hi`; otherwise the bf16 pair.  put_pair is the second half alone, for
// producers whose entry point takes both planes or neither.
template <int N, class P>
__device__ __forceinline__ void put_pair(const float (&v)[N], P* hi, P* lo, size_t o) {
  typename PlaneWords<N>::bf16 h, l;
  split_planes<N>(v, h, l);
  *reinterpret_cast<typename PlaneWords<N>::bf16*>(hi + o) = h;
  *reinterpret_cast<typename PlaneWords<N>::bf16*>(lo + o) = l;
}
template <int N, class P>
__device__ __forceinline__ void put_planes(const float (&v)[N], P* hi, P* lo, size_t o, int shift) {
  if (lo) put_pair<N>(v, hi, lo, o);
  else *reinterpret_cast<typename PlaneWords<N>::f16*>(hi + o) = f16_planes<N>(v, shift);
}
__device__ __forceinline__ void put_pair(const float4& v, unsigned short* hi, unsigned short* lo, size_t o) {
  const float x[4] = {v.x, v.y, v.z, v.w};
  put_pair<4>(x, hi, lo, o);
}
__device__ __forceinline__ void put_planes(const float4& v, unsigned short* hi, unsigned short* lo, size_t o, int shift) {
  const float x[4] = {v.x, v.y, v.z, v.w};
  put_planes<4>(x, hi, lo, o, shift);
}

// The reader: the fp32 values of N plane words at element offset o — hi + lo, or (lo == nullptr) the fp16 word, which
// still carries its 2^shift: the caller takes it off where it wants to.
template <int N, class P>
__device__ __forceinline__ void get_planes(const P* hi, const P* lo, size_t o, float (&v)[N]) {
  if (lo) {
    const typename PlaneWords<N>::bf16 a = *reinterpret_cast<const typename PlaneWords<N>::bf16*>(hi + o),
                                       b = *reinterpret_cast<const typename PlaneWords<N>::bf16*>(lo + o);
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = (float)a[e] + (float)b[e];
  } else {
    const typename PlaneWords<N>::f16 a = *reinterpret_cast<const typename PlaneWords<N>::f16*>(hi + o);
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = (float)a[e];
  }
}

}  // namespace jtsm
