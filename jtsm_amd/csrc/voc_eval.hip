// Pascal VOC detection AP (IoU 0.50:0.05:0.95) and CorLoc on the device: the arithmetic of the reference's
// detectron2/evaluation/pascal_voc_evaluation.py (voc_eval :242-355, voc_ap :210-239, voc_eval_corloc :358-452) on what
// its process() :55-69 prints, without the text files.  Semantics: DESIGN.md §4e.
//
//   quantise  one thread per detection: the score's thousandths q = rint(double(s) * 1000) and the boxes' tenths
//             rint(double(x) * 10) (xmin / ymin after the fp32 `+ 1`) — what f"{s:.3f}" / f"{x:.1f}" print and float()
//             parses back, as integers over 1000.0 / 10.0 — and two sort keys, (class, image, 1023 - q) for matching and
//             (class, 1023 - q) for ranking; the score range for evaluate()'s [0, 1] assertion.
//   sort      hipcub radix sort of both keys over an iota: stable, so equal quantised scores stay in arrival order.
//   match     one wavefront per (class, image) segment of the match order: lanes over the segment's ground-truth boxes
//             in chunks of 64, (overlap, index) wave reduction with the first-maximum rule, detections walked in rank
//             order; the ten thresholds' claimed sets are one 16-bit word per ground-truth box in the workspace.  The
//             segment's first detection settles CorLoc of that image (integer atomics: order-independent).
//   ap        one workgroup per (class, threshold): the class's ranked TP / FP bits in chunks of kApChunk with a block
//             scan carrying the running sums; 11-point and area form.
//
// Everything after the quantisation is fp64.  This file is compiled with -ffp-contract=off (jtsm_amd/build.py): `uni`
// is a*b + c*d - inters, and a fused multiply-add rounds once where the reference rounds twice.
#include <hipcub/hipcub.hpp>

#include <cfloat>
#include <climits>

#include "common.h"

namespace jtsm {
namespace {

typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned short u16;

constexpr int kThr = 10;          // IoU thresholds 0.50 : 0.05 : 0.95
constexpr int kScoreBits = 10;    // 1023 - q, q in [0, 1023]
constexpr int kMaxClassBits = 16, kMaxImageBits = 24;
constexpr int kApChunk = 256;     // detections per step of the AP walk = threads of its workgroup

struct EvalHeader {
  u32 score_max;       // ordered encoding of the largest score
  u32 score_min_inv;   // ~ordered encoding of the smallest score
  u32 pad[2];
};

__device__ __forceinline__ u32 ordered(float f) {
  const u32 u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unordered(u32 e) {
  return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}

__device__ __forceinline__ double thr_of(int t) { return (double)(50 + 5 * t) / 100.0; }

__global__ __launch_bounds__(256) void voc_quantise_kernel(const float4* __restrict__ boxes,
                                                           const float* __restrict__ scores,
                                                           const int* __restrict__ classes,
                                                           const int* __restrict__ images, int D, int N, int C,
                                                           int image_bits, double4* __restrict__ bbq,
                                                           u64* __restrict__ mkey, u64* __restrict__ rkey,
                                                           int* __restrict__ iota, EvalHeader* __restrict__ hdr) {
#pragma clang fp contract(off)
  const int d = blockIdx.x * 256 + threadIdx.x;
  u32 emax = 0, emin_inv = 0;
  if (d < D) {
    const float s = scores[d];
    const double v = rint((double)s * 1000.0);
    const int q = v >= 0.0 ? (v <= 1023.0 ? (int)v : 1023) : 0;      // (NaN -> 0; out of [0, 1] is evaluate()'s error)
    const float4 b = boxes[d];
    const float x0 = b.x + 1.0f, y0 = b.y + 1.0f;                     // the reference's fp32 `xmin += 1`
    double4 o;
    o.x = rint((double)x0 * 10.0) / 10.0;
    o.y = rint((double)y0 * 10.0) / 10.0;
    o.z = rint((double)b.z * 10.0) / 10.0;
    o.w = rint((double)b.w * 10.0) / 10.0;
    bbq[d] = o;
    int c = classes[d], im = images[d];
    if (c < 0 || c >= C || im < 0 || im >= N) { c = C; im = 0; }      // sorted behind every class, never ranked
    const u64 low = (u64)(1023 - q);
    mkey[d] = ((u64)c << (image_bits + kScoreBits)) | ((u64)im << kScoreBits) | low;
    rkey[d] = ((u64)c << kScoreBits) | low;
    iota[d] = d;
    emax = ordered(s);
    emin_inv = ~emax;
  }
  for (int o = 32; o > 0; o >>= 1) {
    emax = max(emax, (u32)__shfl_xor((int)emax, o));
    emin_inv = max(emin_inv, (u32)__shfl_xor((int)emin_inv, o));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&hdr->score_max, emax);
    atomicMax(&hdr->score_min_inv, emin_inv);
  }
}

// start[c] = first rank position of class c, c in [0, C]; start[C] = number of valid detections
__global__ __launch_bounds__(64) void voc_class_start_kernel(const u64* __restrict__ rkey_sorted, int D, int C,
                                                             int* __restrict__ start) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c > C) return;
  const u64 want = (u64)c << kScoreBits;
  int lo = 0, hi = D;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (rkey_sorted[mid] < want) lo = mid + 1; else hi = mid;
  }
  start[c] = lo;
}

// counts[c] = {npos: non-difficult boxes of the class, npos_im: images holding at least one}
__global__ __launch_bounds__(256) void voc_counts_kernel(const unsigned char* __restrict__ difficult,
                                                         const int* __restrict__ offsets, int N, int C,
                                                         int* __restrict__ counts) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)N * C) return;
  const int a = offsets[t], b = offsets[t + 1];
  int nd = 0;
  for (int j = a; j < b; ++j) nd += difficult[j] ? 0 : 1;
  if (nd > 0) {
    const int c = (int)(t / N);
    atomicAdd(&counts[2 * c], nd);
    atomicAdd(&counts[2 * c + 1], 1);
  }
}

__device__ __forceinline__ double overlap(const double4 bb, const int4 g) {
#pragma clang fp contract(off)
  const double g0 = (double)g.x, g1 = (double)g.y, g2 = (double)g.z, g3 = (double)g.w;
  const double ixmin = fmax(g0, bb.x), iymin = fmax(g1, bb.y), ixmax = fmin(g2, bb.z), iymax = fmin(g3, bb.w);
  const double iw = fmax(ixmax - ixmin + 1.0, 0.0), ih = fmax(iymax - iymin + 1.0, 0.0);
  const double inters = iw * ih;
  const double uni = (bb.z - bb.x + 1.0) * (bb.w - bb.y + 1.0) + (g2 - g0 + 1.0) * (g3 - g1 + 1.0) - inters;
  return inters / uni;
}

// One wavefront per position of the match order; the wavefront at the head of a (class, image) segment walks it.
__global__ __launch_bounds__(256) void voc_match_kernel(const u64* __restrict__ mkey, const int* __restrict__ midx,
                                                        int D, int N, int C, int image_bits,
                                                        const double4* __restrict__ bbq,
                                                        const int4* __restrict__ gt_boxes,
                                                        const unsigned char* __restrict__ gt_difficult,
                                                        const int* __restrict__ gt_offsets, u16* __restrict__ claimed,
                                                        int* __restrict__ corloc_cnt, u16* __restrict__ tp_bits,
                                                        u16* __restrict__ fp_bits) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= D) return;
  const u64 seg = mkey[p] >> kScoreBits;
  if (p > 0 && (mkey[p - 1] >> kScoreBits) == seg) return;            // not a segment head (wave-uniform)
  const int c = (int)(seg >> image_bits), im = (int)(seg & ((1ull << image_bits) - 1ull));
  if (c >= C) return;                                                  // the invalid detections' segment
  const int g_lo = gt_offsets[(long)c * N + im], ng = gt_offsets[(long)c * N + im + 1] - g_lo;
  // chunk 0 of the ground truth stays in registers: nearly every segment has no more than 64 boxes
  int4 g_first = make_int4(0, 0, 0, 0);
  if (lane < ng) g_first = gt_boxes[g_lo + lane];
  bool easy = false;                                                   // a non-difficult box in this image?
  for (int j0 = 0; j0 < ng; j0 += 64) {
    const int j = j0 + lane;
    easy = easy || __any(j < ng && gt_difficult[g_lo + j] == 0);
  }
  for (long k = p; k < D && (mkey[k] >> kScoreBits) == seg; ++k) {
    const int d = midx[k];
    const double4 bb = bbq[d];
    double best = -INFINITY;
    int arg = INT_MAX;
    bool nan = false;
    for (int j0 = 0; j0 < ng; j0 += 64) {
      const int j = j0 + lane;
      if (j < ng) {
        const double ov = overlap(bb, j0 == 0 ? g_first : gt_boxes[g_lo + j]);
        if (ov != ov) nan = true;
        else if (ov > best) { best = ov; arg = j; }                    // strict: the earlier chunk keeps a tie
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(best, o);
      const int a = __shfl_xor(arg, o);
      if (ov > best || (ov == best && a < arg)) { best = ov; arg = a; }   // first maximum
    }
    // np.max over a NaN overlap is NaN, and NaN > thr is false; no lane above -inf (an inverted box): nothing to claim
    const bool none = ng == 0 || __any(nan) || arg == INT_MAX;
    if (lane == 0) {
      u16 tp = 0, fp = 0;
      if (none) {
        fp = (1u << kThr) - 1u;
      } else {
        const u16 was = claimed[g_lo + arg];
        const bool diff = gt_difficult[g_lo + arg] != 0;
        u16 now = was;
#pragma unroll
        for (int t = 0; t < kThr; ++t) {
          if (best > thr_of(t)) {
            if (!diff) {
              if (!((was >> t) & 1)) { tp |= (u16)(1u << t); now |= (u16)(1u << t); }
              else fp |= (u16)(1u << t);
            }
            if (k == p && easy) atomicAdd(&corloc_cnt[c * kThr + t], 1);
          } else {
            fp |= (u16)(1u << t);
          }
        }
        if (now != was) claimed[g_lo + arg] = now;
      }
      tp_bits[d] = tp;
      fp_bits[d] = fp;
    }
  }
}

// One workgroup per (class, threshold).
__global__ __launch_bounds__(kApChunk) void voc_ap_kernel(const int* __restrict__ ridx, const int* __restrict__ start,
                                                          const u16* __restrict__ tp_bits,
                                                          const u16* __restrict__ fp_bits,
                                                          const int* __restrict__ counts,
                                                          const int* __restrict__ corloc_cnt, int C, int D,
                                                          int use_07_metric, const EvalHeader* __restrict__ hdr,
                                                          double* __restrict__ ap_out, double* __restrict__ corloc_out,
                                                          double* __restrict__ stats, int* __restrict__ order) {
#pragma clang fp contract(off)
  typedef hipcub::BlockScan<u64, kApChunk> SumScan;
  typedef hipcub::BlockScan<double, kApChunk> MaxScan;
  typedef hipcub::BlockReduce<double, kApChunk> Reduce;
  typedef hipcub::BlockReduce<u64, kApChunk> ReduceU;
  __shared__ union {
    typename SumScan::TempStorage sum;
    typename MaxScan::TempStorage mx;
    typename Reduce::TempStorage red;
    typename ReduceU::TempStorage redu;
  } temp;
  __shared__ double sh_a[kApChunk];
  __shared__ double sh_b[kApChunk];
  __shared__ u64 sh_u;
  const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  const int base = start[c], n = start[c + 1] - base;
  const double npos = (double)counts[2 * c];
  const int nchunk = (n + kApChunk - 1) / kApChunk;

  if (tid == 0) {
    const int npos_im = counts[2 * c + 1];
    corloc_out[t * C + c] = n == 0 ? 0.0 : (npos_im == 0 ? (double)NAN : (double)corloc_cnt[c * kThr + t] / (double)npos_im);
    if (c == 0 && t == 0) {
      stats[0] = D > 0 ? (double)unordered(~hdr->score_min_inv) : 0.0;
      stats[1] = D > 0 ? (double)unordered(hdr->score_max) : 0.0;
      stats[2] = (double)(D - start[C]);      // detections whose class or image index was out of range
      stats[3] = 0.0;
    }
  }

  // packed running sums: TP in the high word, FP in the low word
  auto bits_of = [&](int k) -> u64 {
    const int d = ridx[base + k];
    return ((u64)((tp_bits[d] >> t) & 1) << 32) | (u64)((fp_bits[d] >> t) & 1);
  };
  double ap = 0.0;
  if (use_07_metric) {
    double pm[11];
#pragma unroll
    for (int i = 0; i < 11; ++i) pm[i] = 0.0;
    u64 carry = 0;
    for (int ch = 0; ch < nchunk; ++ch) {
      const int k = ch * kApChunk + tid;
      const bool valid = k < n;
      if (valid && t == 0 && order) order[ridx[base + k]] = k;
      u64 inc;
      SumScan(temp.sum).InclusiveSum(valid ? bits_of(k) : 0ull, inc);
      inc += carry;
      if (tid == kApChunk - 1) sh_u = inc;
      __syncthreads();
      carry = sh_u;
      __syncthreads();
      if (valid) {
        const double tpc = (double)(inc >> 32), fpc = (double)(inc & 0xffffffffull);
        const double rec = tpc / npos, prec = tpc / fmax(tpc + fpc, DBL_EPSILON);
#pragma unroll
        for (int i = 0; i < 11; ++i)
          if (rec >= (double)i * 0.1) pm[i] = fmax(pm[i], prec);
      }
    }
#pragma unroll
    for (int i = 0; i < 11; ++i) {
      const double m = Reduce(temp.red).Reduce(pm[i], hipcub::Max());
      __syncthreads();
      ap = ap + m / 11.0;                      // (thread 0 holds the reduction)
    }
  } else {
    u64 mine = 0;
    for (int k = tid; k < n; k += kApChunk) {
      mine += bits_of(k);
      if (t == 0 && order) order[ridx[base + k]] = k;
    }
    const u64 tot = ReduceU(temp.redu).Sum(mine);
    if (tid == 0) sh_u = tot;
    __syncthreads();
    u64 end = sh_u;                            // running sums at the end of the current chunk
    __syncthreads();
    double env_carry = 0.0;                    // the envelope right of the current chunk (the sentinel 0 at the end)
    for (int ch = nchunk - 1; ch >= 0; --ch) {
      const int k = ch * kApChunk + tid;
      const bool valid = k < n;
      const u64 b = valid ? bits_of(k) : 0ull;
      u64 inc;
      SumScan(temp.sum).InclusiveSum(b, inc);
      if (tid == kApChunk - 1) sh_u = inc;
      __syncthreads();
      const u64 begin = end - sh_u;
      inc += begin;
      const double tpc = (double)(inc >> 32), fpc = (double)(inc & 0xffffffffull);
      const double rec = tpc / npos, prec = valid ? tpc / fmax(tpc + fpc, DBL_EPSILON) : 0.0;
      const double prev = k == 0 ? 0.0 : (double)((inc - b) >> 32) / npos;
      sh_a[tid] = prec;
      __syncthreads();
      double smax;                             // suffix maximum inside the chunk: a prefix scan of the reversed chunk
      MaxScan(temp.mx).InclusiveScan(sh_a[kApChunk - 1 - tid], smax, hipcub::Max());
      sh_b[kApChunk - 1 - tid] = fmax(smax, env_carry);
      __syncthreads();
      const double env = sh_b[tid];
      env_carry = sh_b[0];
      const double term = (valid && rec != prev) ? (rec - prev) * env : 0.0;
      const double s = Reduce(temp.red).Sum(term);
      ap = ap + s;                             // (thread 0)
      end = begin;
      __syncthreads();
    }
  }
  if (tid == 0) ap_out[t * C + c] = ap;
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

int bits_for(long k) {   // bits needed to hold values 0..k
  int b = 1;
  while ((1L << b) <= k) ++b;
  return b;
}

struct EvalLayout {
  size_t zeroed, header, corloc_cnt, claimed, zeroed_end;
  size_t start, mkey_a, mkey_b, rkey_a, rkey_b, iota, midx, ridx, bbq, tp, fp, cub, total;
  size_t cub_bytes;
};

size_t cub_temp_bytes(int D) {
  size_t a = 0;
  u64* k = nullptr;
  int* v = nullptr;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, k, k, v, v, D, 0, 64, (hipStream_t) nullptr);
  return a;
}

EvalLayout eval_layout(int D, int G, int C) {
  EvalLayout l = {};
  const size_t d = D > 0 ? D : 0, g = G > 0 ? G : 0, c = C > 0 ? C : 0;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += align256(bytes ? bytes : 1); return at; };
  l.zeroed = o;
  l.header = take(sizeof(EvalHeader));
  l.corloc_cnt = take(c * kThr * 4);
  l.claimed = take(g * 2);
  l.zeroed_end = o;
  l.start = take((c + 2) * 4);
  l.mkey_a = take(d * 8);
  l.mkey_b = take(d * 8);
  l.rkey_a = take(d * 8);
  l.rkey_b = take(d * 8);
  l.iota = take(d * 4);
  l.midx = take(d * 4);
  l.ridx = take(d * 4);
  l.bbq = take(d * 32);
  l.tp = take(d * 2);
  l.fp = take(d * 2);
  l.cub_bytes = D > 0 ? cub_temp_bytes(D) : 0;
  l.cub = take(l.cub_bytes);
  l.total = o;
  return l;
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" size_t jtsm_voc_eval_workspace_bytes(int D, int G, int C) { return eval_layout(D, G, C).total; }

extern "C" int jtsm_voc_eval(const float* det_boxes, const float* det_scores, const int32_t* det_classes,
                             const int32_t* det_images, int D, const int32_t* gt_boxes, const uint8_t* gt_difficult,
                             const int32_t* gt_offsets, int G, int N, int C, int use_07_metric, double* ap,
                             double* corloc, int32_t* counts, double* stats, uint16_t* tp_bits, uint16_t* fp_bits,
                             int32_t* order, void* workspace, size_t workspace_bytes, void* stream) {
  JTSM_REQUIRE(D >= 0 && G >= 0 && N >= 1 && C >= 1, "voc_eval: D=%d G=%d N=%d C=%d", D, G, N, C);
  JTSM_REQUIRE(C < (1 << kMaxClassBits), "voc_eval: C=%d exceeds the %d class bits of the sort keys (at most %d)", C,
               kMaxClassBits, (1 << kMaxClassBits) - 1);
  JTSM_REQUIRE(N <= (1 << kMaxImageBits), "voc_eval: N=%d exceeds the %d image bits of the sort keys (at most %d)", N,
               kMaxImageBits, 1 << kMaxImageBits);
  JTSM_REQUIRE(ap && corloc && counts && stats && gt_offsets, "voc_eval: null output or gt_offsets");
  JTSM_REQUIRE(D == 0 || (det_boxes && det_scores && det_classes && det_images), "voc_eval: null detections");
  JTSM_REQUIRE(G == 0 || (gt_boxes && gt_difficult), "voc_eval: null ground truth");
  JTSM_REQUIRE(((size_t)det_boxes & 15) == 0 && ((size_t)gt_boxes & 15) == 0, "voc_eval: boxes must be 16-byte aligned");
  const EvalLayout l = eval_layout(D, G, C);
  JTSM_REQUIRE(workspace && workspace_bytes >= l.total && ((size_t)workspace & 255) == 0,
               "voc_eval: workspace of %zu bytes (256-byte aligned) needed", l.total);
  hipStream_t st = as_stream(stream);
  char* ws = static_cast<char*>(workspace);
  EvalHeader* hdr = reinterpret_cast<EvalHeader*>(ws + l.header);
  int* corloc_cnt = reinterpret_cast<int*>(ws + l.corloc_cnt);
  u16* claimed = reinterpret_cast<u16*>(ws + l.claimed);
  int* start = reinterpret_cast<int*>(ws + l.start);
  u64* mkey_a = reinterpret_cast<u64*>(ws + l.mkey_a);
  u64* mkey_b = reinterpret_cast<u64*>(ws + l.mkey_b);
  u64* rkey_a = reinterpret_cast<u64*>(ws + l.rkey_a);
  u64* rkey_b = reinterpret_cast<u64*>(ws + l.rkey_b);
  int* iota = reinterpret_cast<int*>(ws + l.iota);
  int* midx = reinterpret_cast<int*>(ws + l.midx);
  int* ridx = reinterpret_cast<int*>(ws + l.ridx);
  double4* bbq = reinterpret_cast<double4*>(ws + l.bbq);
  u16* tp = tp_bits ? tp_bits : reinterpret_cast<u16*>(ws + l.tp);
  u16* fp = fp_bits ? fp_bits : reinterpret_cast<u16*>(ws + l.fp);
  const int image_bits = bits_for(N - 1), class_bits = bits_for(C);

  JTSM_CHECK_HIP(hipMemsetAsync(ws + l.zeroed, 0, l.zeroed_end - l.zeroed, st));
  JTSM_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)C * 2 * sizeof(int32_t), st));
  hipLaunchKernelGGL(voc_counts_kernel, dim3(ceil_div((long)N * C, 256)), dim3(256), 0, st, gt_difficult, gt_offsets, N,
                     C, counts);
  JTSM_CHECK_LAUNCH("voc counts");
  if (D > 0) {
    JTSM_CHECK_HIP(hipMemsetAsync(tp, 0, (size_t)D * 2, st));        // (detections with an index out of range keep 0 / -1)
    JTSM_CHECK_HIP(hipMemsetAsync(fp, 0, (size_t)D * 2, st));
    if (order) JTSM_CHECK_HIP(hipMemsetAsync(order, 0xff, (size_t)D * 4, st));
    hipLaunchKernelGGL(voc_quantise_kernel, dim3(ceil_div(D, 256)), dim3(256), 0, st,
                       reinterpret_cast<const float4*>(det_boxes), det_scores, det_classes, det_images, D, N, C,
                       image_bits, bbq, mkey_a, rkey_a, iota, hdr);
    JTSM_CHECK_LAUNCH("voc quantise");
    size_t cub_bytes = l.cub_bytes;
    JTSM_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(ws + l.cub, cub_bytes, mkey_a, mkey_b, iota, midx, D, 0,
                                                      kScoreBits + image_bits + class_bits, st));
    cub_bytes = l.cub_bytes;
    JTSM_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(ws + l.cub, cub_bytes, rkey_a, rkey_b, iota, ridx, D, 0,
                                                      kScoreBits + class_bits, st));
  }
  hipLaunchKernelGGL(voc_class_start_kernel, dim3(ceil_div(C + 1, 64)), dim3(64), 0, st, rkey_b, D, C, start);
  JTSM_CHECK_LAUNCH("voc class start");
  if (D > 0) {
    hipLaunchKernelGGL(voc_match_kernel, dim3(ceil_div(D, 4)), dim3(256), 0, st, mkey_b, midx, D, N, C, image_bits, bbq,
                       reinterpret_cast<const int4*>(gt_boxes), gt_difficult, gt_offsets, claimed, corloc_cnt, tp, fp);
    JTSM_CHECK_LAUNCH("voc match");
  }
  hipLaunchKernelGGL(voc_ap_kernel, dim3(C, kThr), dim3(kApChunk), 0, st, ridx, start, tp, fp, counts, corloc_cnt, C, D,
                     use_07_metric, hdr, ap, corloc, stats, order);
  JTSM_CHECK_LAUNCH("voc ap");
  return JTSM_OK;
}
