// What the pseudo-label miners (mining.hip, mist.hip, cmil.hip, pcl.hip) must agree on, one definition each: which
// image a row belongs to, the class score a row is ranked by, the box a mined row stands for, and a rank by counting.
#pragma once
#include "box_math.h"
#include "common.h"

namespace jtsm {

// image of row r, offsets[i] .. offsets[i + 1] being the rows of image i (rows at or past offsets[nimg]: the last)
__device__ __forceinline__ int image_of(const int* __restrict__ offsets, int nimg, int r) {
  int i = 0;
  while (i + 1 < nimg && r >= offsets[i + 1]) ++i;
  return i;
}

// the class score of a row: scores[r, cls], or the soft-max probability exp(scores[r, cls] - lse[r]) when lse is given
__device__ __forceinline__ float class_score(const float* __restrict__ scores, int ld, const float* __restrict__ lse,
                                             int r, int cls) {
  float v = scores[(size_t)r * ld + cls];
  if (lse) v = expf(v - lse[r]);
  return v;
}

// the pseudo box of mined row r for class cls: the class's box decoded from the deltas; without deltas the proposal,
// or (decode_zero: a branch without regression, where the reference decodes zeros) the proposal through decode_box
__device__ __forceinline__ float4 mined_box(const float* __restrict__ proposals, const float* __restrict__ deltas,
                                            int ld_d, int decode_zero, int r, int cls) {
  const float* __restrict__ p = proposals + 4 * (size_t)r;
  float bx[4];
  if (deltas) {
    decode_box(p, deltas + (size_t)r * ld_d + 4 * cls, bx);
  } else if (decode_zero) {
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
    decode_box(p, zero, bx);
  } else {
    for (int k = 0; k < 4; ++k) bx[k] = p[k];
  }
  return make_float4(bx[0], bx[1], bx[2], bx[3]);
}

// A position in a total order is the NUMBER OF KEYS ABOVE one's own — counted, not sorted.  The whole workgroup (of
// THREADS) calls: the list's n keys (key_at(i), 64-bit and distinct: order_key) pass through the LDS `tile` TILE at a
// time, read back as broadcasts, and every thread counts into before[u], for the first own_n (uniform) of its OWN keys,
// the keys above key[u]; a padding key of ~0 has nothing above it.  UNROLL: the unroll hint of the tile walk, 0 for none.
template <int OWN>
__device__ __forceinline__ void count_key(unsigned long long k, const unsigned long long (&key)[OWN], int own_n,
                                          int (&before)[OWN]) {
#pragma unroll
  for (int u = 0; u < OWN; ++u)
    if (u < own_n) before[u] += k > key[u] ? 1 : 0;
}
template <int OWN, int TILE, int THREADS, int UNROLL, class KeyAt>
__device__ __forceinline__ void count_before(int n, KeyAt key_at, const unsigned long long (&key)[OWN], int own_n,
                                             int (&before)[OWN], unsigned long long* __restrict__ tile) {
  int cnt[OWN];                                       // (accumulators of its own: through `before` the walk compiles worse)
#pragma unroll
  for (int u = 0; u < OWN; ++u) cnt[u] = 0;
  for (int t0 = 0; t0 < n; t0 += TILE) {
    const int tn = min(TILE, n - t0);
    __syncthreads();                                  // the previous tile's readers are done
    for (int i = threadIdx.x; i < tn; i += THREADS) tile[i] = key_at(t0 + i);
    __syncthreads();
    if constexpr (UNROLL > 0) {
#pragma unroll UNROLL
      for (int i = 0; i < tn; ++i) count_key<OWN>(tile[i], key, own_n, cnt);
    } else {
      for (int i = 0; i < tn; ++i) count_key<OWN>(tile[i], key, own_n, cnt);
    }
  }
#pragma unroll
  for (int u = 0; u < OWN; ++u) before[u] = cnt[u];
}

}  // namespace jtsm
