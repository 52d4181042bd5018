// The stages of the greedy per-class NMS that do not look at a box: shared by the axis-aligned NMS of postprocess.hip
// and the rotated NMS of rotated_boxes.hip, which differ only in the kernel that fills the IoU bit matrix.
//
// Elements live in a flat array (box, score, class); class == num_classes marks a dropped element.  Stages: 64-bit
// keys (class, descending score) -> radix sort -> class segment starts -> 64x64 IoU bit matrix restricted to W column
// words per row (a class never has more than max_per_class members; the includer's kernel) -> one wavefront per class
// walks its segment -> second radix sort puts the survivors first, by descending score, ties by index.
#pragma once
#include "common.h"

#include <hipcub/hipcub.hpp>

#include <cstdint>

namespace jtsm {
namespace {

typedef unsigned long long u64;

struct NmsHeader {
  int n_valid;      // elements with class < num_classes
  int max_coord;    // order-preserving int image of the largest coordinate among valid boxes
  int num_keep;
  int overflow;     // a class had more members than max_per_class allows
};

__device__ __forceinline__ unsigned ordered_desc(float f) {   // larger float -> smaller key (-0 sorts after +0)
  unsigned u = __float_as_uint(f);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~u;
}
__device__ __forceinline__ int float_to_ordered_int(float f) {
  const int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float ordered_int_to_float(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

__global__ void nms_header_init(NmsHeader* h) {
  h->n_valid = 0;
  h->max_coord = float_to_ordered_int(-INFINITY);
  h->num_keep = 0;
  h->overflow = 0;
}

__device__ __forceinline__ void header_accumulate(NmsHeader* h, bool ok, float cmax) {
  // wave-level reduction, then one atomic per wavefront (integer atomics: order-independent results)
  const u64 b = __ballot(ok);
  int m = ok ? float_to_ordered_int(cmax) : float_to_ordered_int(-INFINITY);
  for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0 && b) {
    atomicAdd(&h->n_valid, __popcll(b));
    atomicMax(&h->max_coord, m);
  }
}

__global__ __launch_bounds__(256) void nms_keys_kernel(const float* __restrict__ escore, const int* __restrict__ eclass,
                                                       int N, u64* __restrict__ key, int* __restrict__ iota) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  key[e] = ((u64)(unsigned)eclass[e] << 32) | ordered_desc(escore[e]);
  iota[e] = e;
}

// seg[c] = first sorted position whose class is >= c, c = 0..K (seg[K] = number of valid elements)
__global__ void nms_segments_kernel(const u64* __restrict__ keys, int N, int K, int* __restrict__ seg) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > K) return;
  int lo = 0, hi = N;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int)(keys[mid] >> 32) < c) lo = mid + 1; else hi = mid;
  }
  seg[c] = lo;
}

__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  const int lo = __shfl((int)(unsigned)(v & 0xffffffffull), src);
  const int hi = __shfl((int)(unsigned)(v >> 32), src);
  return ((u64)(unsigned)hi << 32) | (unsigned)lo;
}

// One wavefront per class walks its segment in score order.  Per 64-row block: the intra-block decisions are made
// from register-resident words (no memory latency in the serial chain), then every lane ORs the kept rows' words
// of one later column block into the LDS-resident `removed` vector (independent loads, all in flight together).
__global__ __launch_bounds__(64) void nms_scan_kernel(const u64* __restrict__ mask, int W,
                                                      const int* __restrict__ seg, uint8_t* __restrict__ kept,
                                                      NmsHeader* h) {
  extern __shared__ u64 removed[];   // 2W words
  const int c = blockIdx.x, lane = threadIdx.x;
  const int s = seg[c], e = seg[c + 1];
  if (s >= e) return;
  const int b0 = s >> 6, b1 = (e - 1) >> 6;
  if (b1 - b0 >= W) {   // more members than the caller promised
    if (lane == 0) atomicExch(&h->overflow, 1);
    return;
  }
  for (int w = lane; w < 2 * W; w += 64) removed[w] = 0;
  __syncthreads();
  int total = 0;
  for (int b = b0; b <= b1; ++b) {
    const int p = b * 64 + lane;
    const bool valid = p >= s && p < e;
    const u64 own = valid ? mask[(size_t)p * W] : 0ull;
    u64 cur = removed[b - b0];
    const u64 vbits = __ballot(valid);
    u64 keptbits = 0;
    for (int j = 0; j < 64; ++j) {
      const u64 o = shfl64(own, j);
      if (((vbits >> j) & 1) && !((cur >> j) & 1)) {
        keptbits |= 1ull << j;
        cur |= o;
      }
    }
    if (valid) kept[p] = (uint8_t)((keptbits >> lane) & 1);
    total += __popcll(keptbits);
    for (int w = 1 + lane; w < W; w += 64) {
      // every row of the block is read (independent loads, all in flight together) and masked by its kept bit:
      // cheaper than a dependent load per kept row
      const u64* col = mask + (size_t)b * 64 * W + w;
      u64 acc = 0;
#pragma unroll 16
      for (int j = 0; j < 64; ++j) acc |= col[(size_t)j * W] & (0ull - ((keptbits >> j) & 1ull));
      removed[b - b0 + w] |= acc;
    }
    __syncthreads();
  }
  if (lane == 0) atomicAdd(&h->num_keep, total);
}

__global__ __launch_bounds__(256) void nms_final_keys_kernel(const int* __restrict__ sidx,
                                                             const uint8_t* __restrict__ kept,
                                                             const float* __restrict__ escore, int N,
                                                             u64* __restrict__ key2) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N) return;
  const int e = sidx[p];
  key2[e] = ((u64)(kept[p] ? 0u : 1u) << 32) | ordered_desc(escore[e]);
}

__global__ __launch_bounds__(256) void nms_emit_keep_kernel(const int* __restrict__ order, int n,
                                                            const NmsHeader* __restrict__ h, int64_t* __restrict__ keep,
                                                            int* __restrict__ num_keep, int* __restrict__ overflow) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keep[i] = order[i];
  if (i == 0) {
    *num_keep = h->num_keep;
    if (overflow) *overflow = h->overflow;
  }
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct NmsLayout {
  int N, W, nblk, K;
  size_t header, ebox, escore, eclass, key_a, key_b, iota, sidx, order, seg, kept, rowvalid, mask, cub, total;
  size_t cub_bytes;
};

size_t cub_temp_bytes(int N) {
  size_t a = 0, b = 0;
  u64* k = nullptr;
  int* v = nullptr;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, k, k, v, v, N, 0, 64, (hipStream_t) nullptr);
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, k, k, v, v, N, 0, 33, (hipStream_t) nullptr);
  return a > b ? a : b;
}

// box_bytes: 16 for an xyxy box, 20 for a rotated (cx, cy, w, h, angle) box
NmsLayout nms_layout(int N, int K, int max_per_class, int R, int box_bytes = 16) {
  NmsLayout l = {};
  l.N = N; l.K = K;
  l.W = ceil_div(max_per_class > 0 ? max_per_class : 1, 64) + 1;
  l.nblk = ceil_div(N > 0 ? N : 1, 64);
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += align256(bytes); return at; };
  l.header = take(sizeof(NmsHeader));
  l.ebox = take((size_t)N * box_bytes);
  l.escore = take((size_t)N * 4);
  l.eclass = take((size_t)N * 4);
  l.key_a = take((size_t)N * 8);
  l.key_b = take((size_t)N * 8);
  l.iota = take((size_t)N * 4);
  l.sidx = take((size_t)N * 4);
  l.order = take((size_t)N * 4);
  l.seg = take((size_t)(K + 2) * 4);
  l.kept = take((size_t)l.nblk * 64);
  l.rowvalid = take((size_t)(R > 0 ? R : 1));
  l.mask = take((size_t)l.nblk * 64 * l.W * 8);
  l.cub_bytes = N > 0 ? cub_temp_bytes(N) : 0;
  l.cub = take(l.cub_bytes);
  l.total = o;
  return l;
}

int bits_for(int k) {   // bits needed to hold values 0..k
  int b = 1;
  while ((1 << b) <= k) ++b;
  return b;
}

// elements already written (ebox / escore / eclass / header); runs sort -> bits -> scan -> sort.
// launch_bits(sorted keys, sorted element indices, header, mask) launches the includer's bit-matrix kernel on a
// (nblk, W) grid of one-wavefront workgroups and returns JTSM_OK or an error code.
template <class LaunchBits>
int nms_stages(char* ws, const NmsLayout& l, hipStream_t st, LaunchBits launch_bits) {
  const int N = l.N, K = l.K;
  NmsHeader* h = reinterpret_cast<NmsHeader*>(ws + l.header);
  float* escore = reinterpret_cast<float*>(ws + l.escore);
  int* eclass = reinterpret_cast<int*>(ws + l.eclass);
  u64* key_a = reinterpret_cast<u64*>(ws + l.key_a);
  u64* key_b = reinterpret_cast<u64*>(ws + l.key_b);
  int* iota = reinterpret_cast<int*>(ws + l.iota);
  int* sidx = reinterpret_cast<int*>(ws + l.sidx);
  int* order = reinterpret_cast<int*>(ws + l.order);
  int* seg = reinterpret_cast<int*>(ws + l.seg);
  uint8_t* kept = reinterpret_cast<uint8_t*>(ws + l.kept);
  u64* mask = reinterpret_cast<u64*>(ws + l.mask);
  size_t cub_bytes = l.cub_bytes;
  hipLaunchKernelGGL(nms_keys_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, st, escore, eclass, N, key_a, iota);
  JTSM_CHECK_LAUNCH("nms keys");
  JTSM_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(ws + l.cub, cub_bytes, key_a, key_b, iota, sidx, N, 0,
                                                    32 + bits_for(K), st));
  hipLaunchKernelGGL(nms_segments_kernel, dim3(ceil_div(K + 1, 64)), dim3(64), 0, st, key_b, N, K, seg);
  JTSM_CHECK_LAUNCH("nms segments");
  const int rc = launch_bits(key_b, sidx, h, mask);
  if (rc) return rc;
  JTSM_CHECK_HIP(hipMemsetAsync(kept, 0, (size_t)l.nblk * 64, st));
  hipLaunchKernelGGL(nms_scan_kernel, dim3(K), dim3(64), (size_t)2 * l.W * sizeof(u64), st, mask, l.W, seg, kept, h);
  JTSM_CHECK_LAUNCH("nms scan");
  hipLaunchKernelGGL(nms_final_keys_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, st, sidx, kept, escore, N, key_a);
  JTSM_CHECK_LAUNCH("nms final keys");
  cub_bytes = l.cub_bytes;
  JTSM_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(ws + l.cub, cub_bytes, key_a, key_b, iota, order, N, 0, 33, st));
  return JTSM_OK;
}

}  // namespace
}  // namespace jtsm
