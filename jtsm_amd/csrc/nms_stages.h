// The stages of the greedy per-class NMS that do not look at a box: shared by the axis-aligned NMS of postprocess.hip
// and the rotated NMS of rotated_boxes.hip, which differ only in the kernel that fills the IoU bit matrix.
//
// Elements live in a flat array (box, score, class); class == num_classes marks a dropped element.  Stages: 64-bit
// keys (class, descending score) -> radix sort -> class segment starts -> 64x64 IoU bit matrix restricted to W column
// words per row (a class never has more than max_per_class members; the includer's kernel) -> one wavefront per class
// walks its segment -> second radix sort puts the survivors first, by descending score, ties by index.
#pragma once
#include "reduce.h"
#include "sorted_segments.h"
#include "workspace.h"

#include <cstdint>

namespace jtsm {
namespace {

struct NmsHeader {
  int n_valid;      // elements with class < num_classes
  unsigned max_coord;   // float_order_bits of the largest coordinate among valid boxes
  int num_keep;
  int overflow;     // a class had more members than max_per_class allows
};

// (score keys: ordered_desc, common.h — larger float -> smaller key, -0 sorts after +0)

__global__ void nms_header_init(NmsHeader* h) {
  h->n_valid = 0;
  h->max_coord = float_order_bits(-INFINITY);
  h->num_keep = 0;
  h->overflow = 0;
}

__device__ __forceinline__ void header_accumulate(NmsHeader* h, bool ok, float cmax) {
  // wave-level reduction, then one atomic per wavefront (integer atomics: order-independent results)
  const u64 b = __ballot(ok);
  const unsigned m = wave_reduce(float_order_bits(ok ? cmax : -INFINITY), Max());
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

struct NmsWs {
  int N, W, nblk, K;
  NmsHeader* header;
  void* ebox;           // N boxes of box_bytes each
  float* escore;
  int* eclass;
  u64 *key_a, *key_b;
  int *iota, *sidx, *order, *seg;
  uint8_t *kept, *rowvalid;
  u64* mask;
  char* cub;
  size_t cub_bytes;
};

// box_bytes: 16 for an xyxy box, 20 for a rotated (cx, cy, w, h, angle) box
NmsWs carve(Arena& a, int N, int K, int max_per_class, int R, int box_bytes = 16) {
  NmsWs w;
  w.N = N; w.K = K;
  w.W = ceil_div(max_per_class > 0 ? max_per_class : 1, 64) + 1;
  w.nblk = ceil_div(N > 0 ? N : 1, 64);
  w.header = a.take<NmsHeader>(1);
  w.ebox = a.take<char>((size_t)N * box_bytes);
  w.escore = a.take<float>(N);
  w.eclass = a.take<int>(N);
  w.key_a = a.take<u64>(N);
  w.key_b = a.take<u64>(N);
  w.iota = a.take<int>(N);
  w.sidx = a.take<int>(N);
  w.order = a.take<int>(N);
  w.seg = a.take<int>(K + 2);
  w.kept = a.take<uint8_t>((size_t)w.nblk * 64);
  w.rowvalid = a.take<uint8_t>(R > 0 ? R : 1);
  w.mask = a.take<u64>((size_t)w.nblk * 64 * w.W);
  w.cub_bytes = N > 0 ? sort_pairs_temp_bytes(N) : 0;
  w.cub = a.take<char>(w.cub_bytes);
  return w;
}

// elements already written (ebox / escore / eclass / header); runs sort -> bits -> scan -> sort.
// launch_bits(sorted keys, sorted element indices, header, mask) launches the includer's bit-matrix kernel on a
// (nblk, W) grid of one-wavefront workgroups and returns JTSM_OK or an error code.
template <class LaunchBits>
int nms_stages(const NmsWs& w, hipStream_t st, LaunchBits launch_bits) {
  const int N = w.N, K = w.K;
  size_t cub_bytes = w.cub_bytes;
  hipLaunchKernelGGL(nms_keys_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, st, w.escore, w.eclass, N, w.key_a, w.iota);
  JTSM_CHECK_LAUNCH("nms keys");
  JTSM_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(w.cub, cub_bytes, w.key_a, w.key_b, w.iota, w.sidx, N, 0,
                                                    32 + bits_for(K), st));
  hipLaunchKernelGGL(segment_starts_kernel, dim3(ceil_div(K + 1, 64)), dim3(64), 0, st, w.key_b, N, K, 32, w.seg);
  JTSM_CHECK_LAUNCH("nms segments");
  const int rc = launch_bits(w.key_b, w.sidx, w.header, w.mask);
  if (rc) return rc;
  JTSM_CHECK_HIP(hipMemsetAsync(w.kept, 0, (size_t)w.nblk * 64, st));
  hipLaunchKernelGGL(nms_scan_kernel, dim3(K), dim3(64), (size_t)2 * w.W * sizeof(u64), st, w.mask, w.W, w.seg, w.kept,
                     w.header);
  JTSM_CHECK_LAUNCH("nms scan");
  hipLaunchKernelGGL(nms_final_keys_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, st, w.sidx, w.kept, w.escore, N,
                     w.key_a);
  JTSM_CHECK_LAUNCH("nms final keys");
  cub_bytes = w.cub_bytes;
  JTSM_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(w.cub, cub_bytes, w.key_a, w.key_b, w.iota, w.order, N, 0, 33, st));
  return JTSM_OK;
}

}  // namespace
}  // namespace jtsm
