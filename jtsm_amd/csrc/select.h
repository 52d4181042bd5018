// The chunked top-k select over a map of floats: the k-th largest value by a radix select on the value's bit pattern,
// four passes over 8-bit digits from the top, nothing read back.  Every workgroup owns a contiguous chunk of elements
// (chunks_of: the one split rule of every chunked pass, the fixed-order sums of reduce.h's fold_chunks included) and
// counts its digits in LDS, one histogram per wavefront: values that crowd into one bin (losses around log C early in
// training, a map of -1) would serialise global histogram atomics.  One workgroup folds the per-workgroup histograms
// and picks the bin (top_bin).  The workspace is the histograms and one SelectState, whatever the number of elements.
// KEY ORDER: ordered_bits (common.h) — -0 = +0 and every NaN on top, as torch.topk ranks them; cut_value gives the
// float back.  What a caller does with the cut (ties to the lower flat index in deeplab_loss.hip, strictly above
// max(cut, 0) in panoptic_deeplab.hip) is the caller's.
// RetinaNet's candidate select (retinanet.hip) is another algorithm — unique 64-bit keys, 16-bit digits, one state
// per (image, level) segment, an early exit, global histograms — and is not a copy of this one.
#pragma once
#include "common.h"

namespace jtsm {
namespace {

constexpr int kChunkThreads = 256;
constexpr int kMaxChunkWgs = 512;      // workgroups of a chunked pass
constexpr int kSelectBins = 256;       // 8-bit digits
constexpr int kSelectSlices = 4;       // slices of the per-workgroup histograms that select_pick_kernel folds side by side

// chunk of workgroup b: elements [b * chunk, min(n, (b + 1) * chunk)), chunk a multiple of kChunkThreads
struct Chunks { int wgs; long chunk; };
inline Chunks chunks_of(long n) {
  Chunks c;
  long tiles = (n + kChunkThreads - 1) / kChunkThreads;
  long per = (tiles + kMaxChunkWgs - 1) / kMaxChunkWgs;
  if (per < 1) per = 1;
  c.chunk = per * kChunkThreads;
  c.wgs = (int)((n + c.chunk - 1) / c.chunk);
  if (c.wgs < 1) c.wgs = 1;
  return c;
}
struct ChunkSpan { long p0, p1; };
__device__ __forceinline__ ChunkSpan chunk_of_wg(long n, long chunk) {
  ChunkSpan s;
  s.p0 = (long)blockIdx.x * chunk;
  s.p1 = s.p0 + chunk < n ? s.p0 + chunk : n;
  return s;
}

struct SelectState {
  unsigned prefix;      // digits chosen so far (high bits of the cut's key)
  unsigned need;        // how many of the elements that match the prefix are still to be taken
  unsigned ties;        // after the last pass: elements equal to the cut
  unsigned pad;
};

// the cut as the float it was (every NaN key is one NaN)
__device__ __forceinline__ float cut_value(unsigned key) {
  return key == 0xffffffffu ? __uint_as_float(0x7fc00000u) : float_from_order_bits(key);
}

// The bin, counted from the top, in which the need-th element lies; `above`: the elements in the bins over it.  Bin 0
// where the bins over it hold fewer than `need` — its own count is not looked at: callers keep need <= the total.
__device__ __forceinline__ int top_bin(const unsigned* __restrict__ hist, unsigned need, unsigned& above) {
  above = 0u;
  int b = kSelectBins - 1;
  for (; b > 0; --b) {
    const unsigned c = hist[b];
    if (above + c >= need) break;
    above += c;
  }
  return b;
}

__global__ void select_init_kernel(SelectState* __restrict__ st, unsigned k) {
  if (threadIdx.x == 0) { st->prefix = 0u; st->need = k; st->ties = 0u; st->pad = 0u; }
}

// digit histogram of the chunk's elements that match the digits chosen so far
__global__ __launch_bounds__(kChunkThreads) void select_hist_kernel(const float* __restrict__ v, long n, long chunk,
                                                                    const SelectState* __restrict__ st, int shift,
                                                                    unsigned* __restrict__ hist) {
  __shared__ unsigned h[kChunkThreads / 64][kSelectBins];
  const int t = threadIdx.x, wv = t >> 6;
  for (int i = t; i < (kChunkThreads / 64) * kSelectBins; i += kChunkThreads) (&h[0][0])[i] = 0u;
  __syncthreads();
  const unsigned prefix = st->prefix;
  const int above = shift + 8;     // bits above this digit must equal the prefix's
  const ChunkSpan c = chunk_of_wg(n, chunk);
  for (long p = c.p0 + t; p < c.p1; p += kChunkThreads) {
    const unsigned key = ordered_bits(v[p]);
    const bool match = above >= 32 || (key >> above) == (prefix >> above);
    if (match) atomicAdd(&h[wv][(key >> shift) & (kSelectBins - 1)], 1u);
  }
  __syncthreads();
  for (int d = t; d < kSelectBins; d += kChunkThreads) {
    unsigned s = 0u;
#pragma unroll
    for (int w = 0; w < kChunkThreads / 64; ++w) s += h[w][d];
    hist[(size_t)blockIdx.x * kSelectBins + d] = s;
  }
}

// one workgroup of kSelectBins x kSelectSlices threads: totals per bin (slice j adds workgroups j, j + kSelectSlices,
// ...; integer sums, any order gives the same), then the bin of the need-th element
__global__ __launch_bounds__(kSelectBins * kSelectSlices) void select_pick_kernel(const unsigned* __restrict__ hist,
                                                                                  int wgs, int shift,
                                                                                  SelectState* __restrict__ st) {
  __shared__ unsigned tot[kSelectSlices][kSelectBins];
  const int d = threadIdx.x % kSelectBins, j = threadIdx.x / kSelectBins;
  unsigned s = 0u;
  for (int b = j; b < wgs; b += kSelectSlices) s += hist[(size_t)b * kSelectBins + d];
  tot[j][d] = s;
  __syncthreads();
  if (j == 0) {
    for (int jj = 1; jj < kSelectSlices; ++jj) s += tot[jj][d];
    tot[0][d] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned above;
    const int bin = top_bin(tot[0], st->need, above);
    st->prefix |= (unsigned)bin << shift;
    st->need -= above;
    st->ties = tot[0][bin];
  }
}

// st->prefix = the key of the k-th largest of v[0 .. n), st->need = how many elements equal to it belong to the k,
// st->ties = how many there are.  1 <= k <= n.  hist: kMaxChunkWgs * kSelectBins words.
inline void launch_select(const float* v, long n, Chunks ch, unsigned k, SelectState* st, unsigned* hist,
                          hipStream_t stream) {
  hipLaunchKernelGGL(select_init_kernel, dim3(1), dim3(64), 0, stream, st, k);
  for (int shift = 24; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(select_hist_kernel, dim3(ch.wgs), dim3(kChunkThreads), 0, stream, v, n, ch.chunk, st, shift, hist);
    hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(kSelectBins * kSelectSlices), 0, stream, hist, ch.wgs, shift,
                       st);
  }
}

}  // namespace
}  // namespace jtsm
