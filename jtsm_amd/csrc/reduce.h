// Wavefront and workgroup reductions, one definition each.  The order is part of the contract: a butterfly inside the
// wavefront from offset 32 down to 1 (both partners form the same value, so every lane ends with it), then the
// per-wave values folded in wave order — float sums that go through here are the same bits on every run and in every
// kernel.  Two more orders are part of the contract, for the sums that have always had them: the LDS halving tree
// (wg_tree_sum: s[t] += s[t + o] for o = THREADS / 2 ... 1) and the fold over a chunked pass's partials (fold_chunks:
// thread t owns consecutive chunks, the threads' sums are added in thread order).  Neither may be swapped for the
// butterfly: the last bits of the fp64 sums would change.  No helper here multiplies and adds, so none carries a
// contraction pragma.
#pragma once
#include <hip/hip_runtime.h>

namespace jtsm {

struct Max {
  __device__ float operator()(float a, float b) const { return fmaxf(a, b); }
  template <class T> __device__ T operator()(T a, T b) const { return a > b ? a : b; }
};
struct Min {
  __device__ float operator()(float a, float b) const { return fminf(a, b); }
};
struct Add {
  template <class T> __device__ T operator()(T a, T b) const { return a + b; }
};

template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_max(float v) { return wave_reduce(v, Max()); }
template <class T> __device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, Add()); }

// Over the workgroup, the same value in every thread.  `slot` is a __shared__ array of one value per wavefront.  NW:
// the workgroup's wavefronts where the caller knows them at compile time (the fold unrolls), 0: from blockDim.
template <int NW = 0, class T, class Op>
__device__ __forceinline__ T wg_reduce(T v, Op op, T* __restrict__ slot) {
  v = wave_reduce(v, op);
  __syncthreads();                       // previous readers of slot are done
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = slot[0];
  const int nw = NW ? NW : blockDim.x >> 6;
  for (int w = 1; w < nw; ++w) r = op(r, slot[w]);
  return r;
}

// ---- the LDS halving tree over a workgroup of THREADS (a power of two): the sum is valid in thread 0.  `s`, `sa`, `sb`:
// __shared__ arrays of THREADS values.  The pair form sums two values behind the same barriers.
template <int THREADS, class T>
__device__ __forceinline__ T wg_tree_sum(T v, T* __restrict__ s) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int o = THREADS / 2; o > 0; o >>= 1) {
    if (t < o) s[t] += s[t + o];
    __syncthreads();
  }
  return s[0];
}
template <int THREADS, class A, class B>
__device__ __forceinline__ void wg_tree_sum(A& a, A* __restrict__ sa, B& b, B* __restrict__ sb) {
  const int t = threadIdx.x;
  sa[t] = a; sb[t] = b;
  __syncthreads();
  for (int o = THREADS / 2; o > 0; o >>= 1) {
    if (t < o) { sa[t] += sa[t + o]; sb[t] += sb[t + o]; }
    __syncthreads();
  }
  a = sa[0]; b = sb[0];
}

// ---- the fold over the `wgs` per-workgroup partials of a chunked pass, by one workgroup of THREADS, for a pair of
// partials (pa[b * stride], pb[b * stride]: those of chunk b): thread t sums its ceil(wgs / THREADS) consecutive
// chunks [fold_span), then thread 0 adds the threads' sums in thread order, in one walk for both.  Thread 0 gets the
// totals (the other threads 0); sa[t], sb[t] (__shared__, THREADS values each) are left holding the sum of the threads
// BEFORE t, the exclusive scan in chunk order that an ordered compaction starts from — valid after the caller's next
// barrier.
struct FoldSpan { int b0, b1; };
template <int THREADS>
__device__ __forceinline__ FoldSpan fold_span(int wgs) {
  const int per = (wgs + THREADS - 1) / THREADS;
  FoldSpan f;
  f.b0 = threadIdx.x * per;
  f.b1 = min(wgs, f.b0 + per);
  return f;
}
template <int THREADS, class A, class B>
__device__ __forceinline__ void fold_chunks(const A* __restrict__ pa, const B* __restrict__ pb, int stride, int wgs,
                                            A* __restrict__ sa, B* __restrict__ sb, A& total_a, B& total_b) {
  const FoldSpan f = fold_span<THREADS>(wgs);
  A a = 0;
  B b = 0;
  for (int c = f.b0; c < f.b1; ++c) { a += pa[(size_t)c * stride]; b += pb[(size_t)c * stride]; }
  sa[threadIdx.x] = a; sb[threadIdx.x] = b;
  __syncthreads();
  total_a = 0; total_b = 0;
  if (threadIdx.x == 0)
    for (int i = 0; i < THREADS; ++i) {
      a = sa[i]; b = sb[i];
      sa[i] = total_a; sb[i] = total_b;
      total_a += a; total_b += b;
    }
}

// ---- arg-best over (float value, int index): the larger value wins, the lower index among equal values.  The pair
// travels as one 64-bit word (value bits high, index low) so that it shuffles and sits in a slot like any other value,
// but it is COMPARED AS A FLOAT AND AN INT: -0 equals +0, and a NaN never beats anything — a thread that only takes
// `v > best` never offers one.  (order_key, common.h, is the other rule: NaN first, as torch.topk ranks it.)
// A thread with nothing to offer passes (its start value, kNoIndex).
typedef unsigned long long BestPair;
constexpr int kNoIndex = 0x7fffffff;
__device__ __forceinline__ BestPair best_pair(float v, int index) {
  return ((BestPair)__float_as_uint(v) << 32) | (unsigned)index;
}
__device__ __forceinline__ float best_value(BestPair p) { return __uint_as_float((unsigned)(p >> 32)); }
__device__ __forceinline__ int best_index(BestPair p) { return (int)(unsigned)(p & 0xffffffffull); }
struct ArgBest {
  __device__ BestPair operator()(BestPair a, BestPair b) const {
    const float va = best_value(a), vb = best_value(b);
    return (vb > va || (vb == va && best_index(b) < best_index(a))) ? b : a;
  }
};
template <int NW = 0>
__device__ __forceinline__ BestPair wg_arg_best(float v, int index, BestPair* __restrict__ slot) {
  return wg_reduce<NW>(best_pair(v, index), ArgBest(), slot);
}

// ---- shuffles of values wider than a register
__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src) {
  const int lo = __shfl((int)(unsigned)(v & 0xffffffffull), src);
  const int hi = __shfl((int)(unsigned)(v >> 32), src);
  return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ float4 shfl_box(const float4& v, int src) {
  return make_float4(__shfl(v.x, src), __shfl(v.y, src), __shfl(v.z, src), __shfl(v.w, src));
}

}  // namespace jtsm
