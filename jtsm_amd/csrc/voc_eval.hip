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
//             scan carrying the running sums; 11-point and area form (the latter's chunk step: eval_walk.h).
// Key width, sort scratch and class starts: sorted_segments.h; the workspace: carve() below, over workspace.h's Arena.
//
// Everything after the quantisation is fp64.  This file is compiled with -ffp-contract=off (jtsm_amd/build.py): `uni`
// is a*b + c*d - inters, and a fused multiply-add rounds once where the reference rounds twice.
#include <cfloat>
#include <climits>

#include "eval_walk.h"
#include "sorted_segments.h"
#include "workspace.h"

namespace jtsm {
namespace {

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
    emax = float_order_bits(s);
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
  typedef RankedWalk<kApChunk> Walk;              // (eval_walk.h)
  typedef hipcub::BlockReduce<double, kApChunk> Reduce;
  typedef hipcub::BlockReduce<u64, kApChunk> ReduceU;
  __shared__ union {
    typename Walk::Temp walk;
    typename Reduce::TempStorage red;
    typename ReduceU::TempStorage redu;
  } temp;
  __shared__ typename Walk::Shared sh;
  const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  const int base = start[c], n = start[c + 1] - base;
  const double npos = (double)counts[2 * c];
  const int nchunk = (n + kApChunk - 1) / kApChunk;

  if (tid == 0) {
    const int npos_im = counts[2 * c + 1];
    corloc_out[t * C + c] = n == 0 ? 0.0 : (npos_im == 0 ? (double)NAN : (double)corloc_cnt[c * kThr + t] / (double)npos_im);
    if (c == 0 && t == 0) {
      stats[0] = D > 0 ? (double)float_from_order_bits(~hdr->score_min_inv) : 0.0;
      stats[1] = D > 0 ? (double)float_from_order_bits(hdr->score_max) : 0.0;
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
      typename Walk::SumScan(temp.walk.sum).InclusiveSum(valid ? bits_of(k) : 0ull, inc);
      inc += carry;
      if (tid == kApChunk - 1) sh.u = inc;
      __syncthreads();
      carry = sh.u;
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
    if (tid == 0) sh.u = tot;
    __syncthreads();
    u64 end = sh.u;                            // running sums at the end of the current chunk
    __syncthreads();
    double env_carry = 0.0;                    // the envelope right of the current chunk (the sentinel 0 at the end)
    for (int ch = nchunk - 1; ch >= 0; --ch) {
      const int k = ch * kApChunk + tid;
      const bool valid = k < n;
      const u64 b = valid ? bits_of(k) : 0ull;
      const u64 inc = Walk::running_sum(temp.walk, sh, b, end);      // (one barrier; `end` is now the chunk's begin)
      const double tpc = (double)(inc >> 32), fpc = (double)(inc & 0xffffffffull);
      const double rec = tpc / npos, prec = valid ? tpc / fmax(tpc + fpc, DBL_EPSILON) : 0.0;
      const double prev = k == 0 ? 0.0 : (double)((inc - b) >> 32) / npos;
      const double env = Walk::envelope(temp.walk, sh, prec, env_carry);          // (two barriers)
      const double term = (valid && rec != prev) ? (rec - prev) * env : 0.0;
      const double s = Reduce(temp.red).Sum(term);
      ap = ap + s;                             // (thread 0)
      __syncthreads();                         // temp and sh are free for the next chunk
    }
  }
  if (tid == 0) ap_out[t * C + c] = ap;
}

struct EvalWs {
  size_t zeroed, zeroed_end;        // arena marks around header, corloc_cnt and claimed: cleared by one memset
  EvalHeader* header;
  int* corloc_cnt;
  u16* claimed;
  int* start;
  u64 *mkey_a, *mkey_b, *rkey_a, *rkey_b;
  int *iota, *midx, *ridx;
  double4* bbq;
  u16 *tp, *fp;
  char* cub;
  size_t cub_bytes;
};

EvalWs carve(Arena& a, int D, int G, int C) {
  const size_t d = D > 0 ? D : 0, g = G > 0 ? G : 0, c = C > 0 ? C : 0;
  a.pad_empty = true;
  EvalWs w;
  w.zeroed = a.mark();
  w.header = a.take<EvalHeader>(1);
  w.corloc_cnt = a.take<int>(c * kThr);
  w.claimed = a.take<u16>(g);
  w.zeroed_end = a.mark();
  w.start = a.take<int>(c + 2);
  w.mkey_a = a.take<u64>(d);
  w.mkey_b = a.take<u64>(d);
  w.rkey_a = a.take<u64>(d);
  w.rkey_b = a.take<u64>(d);
  w.iota = a.take<int>(d);
  w.midx = a.take<int>(d);
  w.ridx = a.take<int>(d);
  w.bbq = a.take<double4>(d);
  w.tp = a.take<u16>(d);
  w.fp = a.take<u16>(d);
  w.cub_bytes = D > 0 ? sort_pairs_temp_bytes(D) : 0;
  w.cub = a.take<char>(w.cub_bytes);
  return w;
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" size_t jtsm_voc_eval_workspace_bytes(int D, int G, int C) {
  Arena a{nullptr};
  carve(a, D, G, C);
  return a.off;
}

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
  Arena arena{static_cast<char*>(workspace)};
  const EvalWs w = carve(arena, D, G, C);
  JTSM_REQUIRE(workspace && workspace_bytes >= arena.off && ((size_t)workspace & 255) == 0,
               "voc_eval: workspace of %zu bytes (256-byte aligned) needed", arena.off);
  hipStream_t st = as_stream(stream);
  u16* tp = tp_bits ? tp_bits : w.tp;
  u16* fp = fp_bits ? fp_bits : w.fp;
  const int image_bits = bits_for(N - 1), class_bits = bits_for(C);

  JTSM_CHECK_HIP(hipMemsetAsync(arena.base + w.zeroed, 0, w.zeroed_end - w.zeroed, st));
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
                       image_bits, w.bbq, w.mkey_a, w.rkey_a, w.iota, w.header);
    JTSM_CHECK_LAUNCH("voc quantise");
    size_t cub_bytes = w.cub_bytes;
    JTSM_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(w.cub, cub_bytes, w.mkey_a, w.mkey_b, w.iota, w.midx, D, 0,
                                                      kScoreBits + image_bits + class_bits, st));
    cub_bytes = w.cub_bytes;
    JTSM_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(w.cub, cub_bytes, w.rkey_a, w.rkey_b, w.iota, w.ridx, D, 0,
                                                      kScoreBits + class_bits, st));
  }
  hipLaunchKernelGGL(segment_starts_kernel, dim3(ceil_div(C + 1, 64)), dim3(64), 0, st, w.rkey_b, D, C, kScoreBits,
                     w.start);
  JTSM_CHECK_LAUNCH("voc class start");
  if (D > 0) {
    hipLaunchKernelGGL(voc_match_kernel, dim3(ceil_div(D, 4)), dim3(256), 0, st, w.mkey_b, w.midx, D, N, C, image_bits,
                       w.bbq, reinterpret_cast<const int4*>(gt_boxes), gt_difficult, gt_offsets, w.claimed, w.corloc_cnt,
                       tp, fp);
    JTSM_CHECK_LAUNCH("voc match");
  }
  hipLaunchKernelGGL(voc_ap_kernel, dim3(C, kThr), dim3(kApChunk), 0, st, w.ridx, w.start, tp, fp, counts,
                     w.corloc_cnt, C, D, use_07_metric, w.header, ap, corloc, stats, order);
  JTSM_CHECK_LAUNCH("voc ap");
  return JTSM_OK;
}
