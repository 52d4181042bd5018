// One step of the right-to-left walk over a class's ranked records, CHUNK records = CHUNK threads at a time: what
// voc_ap_kernel's area form and coco_pr_kernel's second pass do per chunk and threshold.
//
//   for chunk from the last to the first:
//     inc = running_sum(word, end)      this record's inclusive tp / fp counts; `end` moves to the chunk's begin
//     prec = the caller's formula on inc
//     env = envelope(prec, carry)       the largest precision at or right of this record
//     ... the caller's use of env ...
//     __syncthreads()                   THE CALLER'S: the next running_sum reuses `temp` and `u`
//
// Barriers: each function holds exactly the barriers written in it; `temp` (the caller's union, which may hold further
// hipcub storage) is free for another use after running_sum returns and after envelope returns, and needs a barrier
// before the use after that.  Both includers are built with -ffp-contract=off; nothing here multiplies and adds.
#pragma once
#include <hipcub/hipcub.hpp>

namespace jtsm {

template <int CHUNK>
struct RankedWalk {
  typedef unsigned long long u64;
  typedef hipcub::BlockScan<u64, CHUNK> SumScan;
  typedef hipcub::BlockScan<double, CHUNK> MaxScan;
  union Temp {
    typename SumScan::TempStorage sum;
    typename MaxScan::TempStorage mx;
  };
  struct Shared {
    double a[CHUNK], b[CHUNK];
    u64 u;
  };

  // word: this thread's tp << 32 | fp (0 past the end); end: the running sums at the chunk's right end on entry, at its
  // begin on return.  Returns the running sums up to and including this thread.
  static __device__ __forceinline__ u64 running_sum(Temp& temp, Shared& sh, u64 word, u64& end) {
    u64 inc;
    SumScan(temp.sum).InclusiveSum(word, inc);
    if (threadIdx.x == CHUNK - 1) sh.u = inc;
    __syncthreads();
    end -= sh.u;
    return inc + end;
  }

  // prec: this thread's precision (0 past the end); carry: the envelope right of the chunk on entry, from the chunk's
  // first record on return.  Returns max(prec of this thread and of every thread right of it, carry): a prefix max-scan
  // of the reversed chunk.
  static __device__ __forceinline__ double envelope(Temp& temp, Shared& sh, double prec, double& carry) {
    const int tid = threadIdx.x;
    sh.a[tid] = prec;
    __syncthreads();
    double smax;
    MaxScan(temp.mx).InclusiveScan(sh.a[CHUNK - 1 - tid], smax, hipcub::Max());
    sh.b[CHUNK - 1 - tid] = fmax(smax, carry);
    __syncthreads();
    carry = sh.b[0];
    return sh.b[tid];
  }
};

}  // namespace jtsm
