// What the stages that radix-sort 64-bit keys (class in the top bits) over an iota share: the key width, the sort's
// scratch size and the class segment starts of the sorted keys.
#pragma once
#include <hipcub/hipcub.hpp>

#include "common.h"

namespace jtsm {
namespace {

typedef unsigned long long u64;

int bits_for(long k) {   // bits needed to hold values 0..k
  int b = 1;
  while ((1L << b) <= k) ++b;
  return b;
}

// Scratch bytes of hipcub::DeviceRadixSort::SortPairs over n (u64 key, int value) pairs, for any bit range: asked for
// all 64 bits, and rocPRIM's scratch only grows with the bit count (one histogram per digit place beside buffers sized
// by n), so a sort over fewer bits fits.  Up to 1024 items the answer is a fixed 256 (one block sorts them); above, it
// follows the device's tuning.  The query's status is dropped on purpose and a FAILED QUERY YIELDS 0: a host without a
// device answers 256 below 4096 items and fails from there on, so a workspace size asked for on such a host lacks the
// sort's scratch (and the sort, which needs a device anyway, would refuse it).
size_t sort_pairs_temp_bytes(int n) {
  size_t bytes = 0;
  u64* k = nullptr;
  int* v = nullptr;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, k, k, v, v, n, 0, 64, (hipStream_t) nullptr);
  return bytes;
}

// start[c] = first position of the ascending keys whose key is >= c << shift, c in [0, K]: the start of class c's
// segment; start[K] = the number of keys below class K (the valid ones).  One thread per c.
__global__ __launch_bounds__(64) void segment_starts_kernel(const u64* __restrict__ sorted_keys, int n, int K, int shift,
                                                            int* __restrict__ start) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c > K) return;
  const u64 want = (u64)c << shift;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (sorted_keys[mid] < want) lo = mid + 1; else hi = mid;
  }
  start[c] = lo;
}

}  // namespace
}  // namespace jtsm
