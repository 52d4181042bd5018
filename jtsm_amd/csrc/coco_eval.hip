// COCO box / mask / keypoint AP on the device: what the reference's COCOEvaluator
// (detectron2/evaluation/coco_evaluation.py) gets from COCOeval_opt (evaluation/fast_eval_api.py) — pycocotools'
// parameters, IoU and OKS, and the reference's own
// detectron2/layers/csrc/cocoeval/cocoeval.cpp for the matching (MatchDetectionsToGroundTruth :61-140) and the
// precision / recall tables (BuildSortedDetectionList :223-273, ComputePrecisionRecallCurve :284-371).
// Semantics: DESIGN.md §4g.
//
//   jtsm_coco_image, one image and one task per call (the masks of a whole dataset cannot stay on the device):
//     rank     one thread per detection: its counted rank inside its category (descending score, ties in row order),
//              its XYWH box and area in fp64 (w, h subtracted in fp32 first), its record;
//     pack     segm: (n, H, W) bytes -> 64-bit words by wave ballot, areas by popcount (one integer atomic per wave);
//     iou      bbox: one thread per (detection, ground truth) pair; segm: one workgroup per pair sums popcount(a & b);
//              keypoints (jtsm_coco_image_keypoints): one thread per pair, pycocotools' computeOks;
//              pairs of different categories and detections past max_det leave on a uniform branch;
//     match    one wavefront per (category, area range, threshold): detections in rank order, lanes over the
//              category's ground truth in chunks of 64, last-maximum arg-max in two phases (non-ignored, then ignored);
//              the matched set is one bit per chunk in a lane's register; results are OR-ed into the records' words.
//   jtsm_coco_accumulate over the concatenated records:
//     key      (category, descending score, image index, rank) -> one hipcub radix sort over the bits in use;
//     start    category starts by binary search (sorted_segments.h);
//     pr       one workgroup per (category, area range, maxDet): totals, then the chunks from the right with a block scan
//              of tp / fp and a reversed max scan for the envelope, all ten thresholds per chunk; the record that first
//              reaches a recall threshold writes its precision and score (the chunk step: eval_walk.h).
// Workspaces: carve_image() / carve_acc() below, over workspace.h's Arena.
//
// fp64 arithmetic only in single correctly rounded operations in the reference's order; compiled with
// -ffp-contract=off (jtsm_amd/build.py): the box IoU's `da + ga - i` after `w * h` must not fuse.
#include <climits>

#include "eval_walk.h"
#include "sorted_segments.h"
#include "workspace.h"

namespace jtsm {
namespace {

typedef unsigned int u32;

constexpr int kT = 10;            // IoU thresholds
constexpr int kA = 4;             // area ranges
constexpr int kRankBits = 7;      // rank inside (image, category): max_det <= 128
constexpr int kMaxDet = 1 << kRankBits;
constexpr int kMaxM = 8;          // maxDets entries
constexpr int kMaxR = 1024;       // recall thresholds
constexpr int kChunk = 256;       // records per step of the precision / recall walk = threads of its workgroup
constexpr int kMaxGtChunks = 64;  // ground truth of one category in one image: 64 chunks of 64 (a lane's matched word)
constexpr int kMaxKeypoints = 64; // keypoints of an object (the OKS thread walks them twice)

struct Record {                   // 32 bytes; the Python side holds them as (D, 4) int64
  int cat;                        // num_categories for a detection that is left out (past max_det, or a bad class)
  int image;
  int rank;
  float score;
  u64 matched;                    // bit a * kT + t: matched to a ground truth at (area range a, threshold t)
  u64 ignore;                     // bit a * kT + t: ignored there
};

// One thread per detection.  cat_count zeroed by the caller.
__global__ __launch_bounds__(256) void coco_rank_kernel(const float4* __restrict__ boxes,
                                                        const float* __restrict__ scores,
                                                        const int* __restrict__ classes, int n, int K, int image,
                                                        int max_det, int segm, double4* __restrict__ dbox,
                                                        double* __restrict__ darea, int* __restrict__ rank_out,
                                                        int* __restrict__ cat_count, int* __restrict__ det_of,
                                                        Record* __restrict__ rec, u64* __restrict__ stats) {
#pragma clang fp contract(off)
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= n) return;
  const int c = classes[d];
  const float s = scores[d];
  const bool ok = c >= 0 && c < K;
  int r = 0;
  if (ok) {
    // compared through the sort key's encoding (the order of the floats, the two zeros equal): a total order even
    // for a NaN, so the ranks of a category are always a permutation
    const u32 ks = float_order_bits(s + 0.0f);
    for (int e = 0; e < n; ++e) {
      const u32 ke = float_order_bits(scores[e] + 0.0f);
      if (classes[e] == c && (ke > ks || (ke == ks && e < d))) ++r;
    }
    atomicAdd(&cat_count[c], 1);
  } else {
    atomicAdd(&stats[0], 1ull);
  }
  const bool keep = ok && r < max_det;
  const float4 b = boxes[d];
  const float w = b.z - b.x, h = b.w - b.y;                     // BoxMode.convert on the fp32 array
  double4 o;
  o.x = (double)b.x; o.y = (double)b.y; o.z = (double)w; o.w = (double)h;
  dbox[d] = o;
  if (!segm) darea[d] = o.z * o.w;
  rank_out[d] = keep ? r : -1;
  if (keep) det_of[(long)c * max_det + r] = d;
  Record out;
  out.cat = keep ? c : K;
  out.image = image;
  out.rank = keep ? r : 0;
  out.score = s;
  out.matched = 0;
  out.ignore = 0;
  rec[d] = out;
}

// grid (blocks per mask, n), 256 threads: wave w of the mask's grid packs words w, w + waves, ...  area zeroed by the
// caller.
__global__ __launch_bounds__(256) void coco_pack_kernel(const unsigned char* __restrict__ masks, long HW, long W64,
                                                        u64* __restrict__ words, int* __restrict__ area) {
  const int d = blockIdx.y, lane = threadIdx.x & 63;
  const unsigned char* m = masks + (long)d * HW;
  u64* out = words + (long)d * W64;
  const long waves = (long)gridDim.x * 4;
  int cnt = 0;
  for (long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6); w < W64; w += waves) {      // (wave-uniform)
    const long p = w * 64 + lane;
    const bool on = p < HW && m[p] != 0;
    const u64 bits = __ballot(on);
    if (lane == 0) out[w] = bits;
    cnt += __popcll(bits);
  }
  if (lane == 0 && cnt) atomicAdd(&area[d], cnt);
}

__global__ __launch_bounds__(256) void coco_area_to_double_kernel(const int* __restrict__ area, int n,
                                                                  double* __restrict__ darea) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d < n) darea[d] = (double)area[d];
}

// category of ground-truth row g from the CSR over categories
__device__ __forceinline__ int gt_cat_of(const int* __restrict__ cat_start, int K, int g) {
  int lo = 0, hi = K;                                            // the c with cat_start[c] <= g < cat_start[c + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (cat_start[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// pycocotools' bbIou on XYWH doubles.  One thread per (d, g).
__global__ __launch_bounds__(256) void coco_box_iou_kernel(const double4* __restrict__ dbox,
                                                           const int* __restrict__ classes,
                                                           const int* __restrict__ rank, int n,
                                                           const double4* __restrict__ gbox,
                                                           const unsigned char* __restrict__ gcrowd,
                                                           const int* __restrict__ cat_start, int K, int G,
                                                           double* __restrict__ ious) {
#pragma clang fp contract(off)
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)n * G) return;
  const int d = (int)(t / G), g = (int)(t % G);
  double o = -1.0;
  if (rank[d] >= 0 && gt_cat_of(cat_start, K, g) == classes[d]) {
    const double4 a = dbox[d], b = gbox[g];
    const double ga = b.z * b.w;
    const double da = a.z * a.w;
    o = 0.0;
    const double w = fmin(a.z + a.x, b.z + b.x) - fmax(a.x, b.x);
    if (w > 0) {
      const double h = fmin(a.w + a.y, b.w + b.y) - fmax(a.y, b.y);
      if (h > 0) {
        const double i = w * h;
        const double s = da + ga;
        const double u = gcrowd[g] ? da : s - i;
        o = i / u;
      }
    }
  }
  ious[t] = o;
}

// pycocotools' rleIou on packed bitmasks.  grid (G, n): one workgroup per pair.
__global__ __launch_bounds__(256) void coco_mask_iou_kernel(const u64* __restrict__ dwords,
                                                            const int* __restrict__ darea_i,
                                                            const int* __restrict__ classes,
                                                            const int* __restrict__ rank,
                                                            const u64* __restrict__ gwords,
                                                            const unsigned char* __restrict__ gcrowd,
                                                            const int* __restrict__ cat_start, int K, int G, long W64,
                                                            double* __restrict__ ious) {
  __shared__ long long sh_i[4], sh_g[4];
  const int g = blockIdx.x, d = blockIdx.y, tid = threadIdx.x;
  const long at = (long)d * G + g;
  if (rank[d] < 0 || gt_cat_of(cat_start, K, g) != classes[d]) {         // (block-uniform)
    if (tid == 0) ious[at] = -1.0;
    return;
  }
  const u64* a = dwords + (long)d * W64;
  const u64* b = gwords + (long)g * W64;
  long long ci = 0, cg = 0;
  for (long w = tid; w < W64; w += 256) {
    const u64 y = b[w];
    ci += __popcll(a[w] & y);
    cg += __popcll(y);
  }
  for (int o = 32; o > 0; o >>= 1) { ci += __shfl_xor(ci, o); cg += __shfl_xor(cg, o); }
  if ((tid & 63) == 0) { sh_i[tid >> 6] = ci; sh_g[tid >> 6] = cg; }
  __syncthreads();
  if (tid == 0) {
    const long long i = sh_i[0] + sh_i[1] + sh_i[2] + sh_i[3], ag = sh_g[0] + sh_g[1] + sh_g[2] + sh_g[3];
    const long long ad = darea_i[d];
    double o = 0.0;
    if (i != 0) {
      const long long u = gcrowd[g] ? ad : ad + ag - i;
      o = (double)i / (double)u;
    }
    ious[at] = o;
  }
}

// pycocotools' computeOks.  One thread per (d, g).  The detection's x and y get instances_to_coco_json's `- 0.5` in
// fp32 where they are read; the sum runs in keypoint order.
__global__ __launch_bounds__(256) void coco_oks_kernel(const float* __restrict__ dkp, const int* __restrict__ classes,
                                                       const int* __restrict__ rank, int n,
                                                       const double4* __restrict__ gbox,
                                                       const double* __restrict__ garea,
                                                       const double* __restrict__ gkp,
                                                       const double* __restrict__ sigmas, int P,
                                                       const int* __restrict__ cat_start, int K, int G,
                                                       double* __restrict__ ious) {
#pragma clang fp contract(off)
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)n * G) return;
  const int d = (int)(t / G), g = (int)(t % G);
  double o = -1.0;
  if (rank[d] >= 0 && gt_cat_of(cat_start, K, g) == classes[d]) {
    const float* a = dkp + (long)d * P * 3;
    const double* b = gkp + (long)g * P * 3;
    int k1 = 0;
    for (int p = 0; p < P; ++p) k1 += b[3 * p + 2] > 0 ? 1 : 0;
    const double4 bb = gbox[g];
    const double x0 = bb.x - bb.z, x1 = bb.x + bb.z * 2;
    const double y0 = bb.y - bb.w, y1 = bb.y + bb.w * 2;
    const double ar = garea[g] + 2.220446049250313e-16;                  // np.spacing(1)
    double sum = 0.0;
    for (int p = 0; p < P; ++p) {
      if (k1 > 0 && !(b[3 * p + 2] > 0)) continue;
      const double xd = (double)(a[3 * p] - 0.5f), yd = (double)(a[3 * p + 1] - 0.5f);
      double dx, dy;
      if (k1 > 0) {
        dx = xd - b[3 * p];
        dy = yd - b[3 * p + 1];
      } else {                                                           // the distance to the doubled box
        dx = fmax(0.0, x0 - xd) + fmax(0.0, xd - x1);
        dy = fmax(0.0, y0 - yd) + fmax(0.0, yd - y1);
      }
      const double s2 = sigmas[p] * 2;
      const double var = s2 * s2;
      const double xx = dx * dx, yy = dy * dy;
      const double e = (xx + yy) / var / ar / 2;
      sum = sum + exp(-e);
    }
    o = sum / (double)(k1 > 0 ? k1 : P);
  }
  ious[t] = o;
}

// One wavefront per (category, area range, threshold); 4 per workgroup.  gignore: the annotation's ignore flag (never
// counted, a match is ignored); gcrowd: may be matched again (cocoeval.cpp:96).  bbox and segm: the same array.
__global__ __launch_bounds__(256) void coco_match_kernel(const int* __restrict__ cat_count,
                                                         const int* __restrict__ det_of,
                                                         const double* __restrict__ darea, int n, int max_det,
                                                         const double* __restrict__ garea,
                                                         const unsigned char* __restrict__ gignore,
                                                         const unsigned char* __restrict__ gcrowd,
                                                         const int* __restrict__ cat_start, int K, int G,
                                                         const double* __restrict__ ious,
                                                         const double* __restrict__ iou_thrs,
                                                         const double* __restrict__ area_rng,
                                                         Record* __restrict__ rec, u64* __restrict__ npos) {
  const int lane = threadIdx.x & 63;
  const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= (long)K * kA * kT) return;
  const int c = (int)(wid / (kA * kT)), a = (int)(wid % (kA * kT)) / kT, t = (int)(wid % kT);
  const int g_lo = cat_start[c], ng = cat_start[c + 1] - g_lo;
  const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
  const int nchunk = (ng + 63) / 64;                                     // (<= kMaxGtChunks: checked by the host)
  // this lane's ground truth: chunk j -> row g_lo + 64 j + lane; one bit per chunk
  u64 ign = 0, crowd = 0, matched = 0;
  int valid = 0;
  for (int j = 0; j < nchunk; ++j) {
    const int g = j * 64 + lane;
    if (g < ng) {
      const bool cr = gcrowd[g_lo + g] != 0;
      const double ar = garea[g_lo + g];
      const bool ig = gignore[g_lo + g] != 0 || ar < lo || ar > hi;
      if (ig) ign |= 1ull << j;
      if (cr) crowd |= 1ull << j;
      if (!ig) ++valid;
    }
  }
  if (t == 0) {
    for (int o = 32; o > 0; o >>= 1) valid += __shfl_xor(valid, o);
    if (lane == 0 && valid) atomicAdd(&npos[c * kA + a], (u64)valid);
  }
  const int nd = min(cat_count[c], max_det);
  if (nd == 0) return;
  const double best0 = fmin(iou_thrs[t], 1 - 1e-10);
  const int bit = a * kT + t;
  for (int r = 0; r < nd; ++r) {
    const int d = det_of[(long)c * max_det + r];
    if (d < 0 || d >= n) continue;                                       // (cannot happen: the ranks are a permutation)
    const double* row = ious + (long)d * G + g_lo;
    int match = -1;
    for (int phase = 0; phase < 2 && match < 0; ++phase) {               // 0: non-ignored, 1: ignored (wave-uniform)
      double best = best0;
      int arg = -1;
      for (int j = 0; j < nchunk; ++j) {
        const int g = j * 64 + lane;
        if (g < ng && (int)((ign >> j) & 1) == phase && !(((matched >> j) & 1) && !((crowd >> j) & 1))) {
          const double v = row[g];
          if (v >= best) { best = v; arg = g; }                          // the later chunk takes a tie
        }
      }
      for (int o = 32; o > 0; o >>= 1) {
        const double v = __shfl_xor(best, o);
        const int g = __shfl_xor(arg, o);
        if (g >= 0 && (arg < 0 || v > best || (v == best && g > arg))) { best = v; arg = g; }   // last maximum
      }
      match = arg;
    }
    bool ignored;
    if (match >= 0) {
      const int j = match >> 6, owner = match & 63;
      ignored = ((u64)__shfl((long long)ign, owner) >> j) & 1;
      if (lane == owner) matched |= 1ull << j;
    } else {
      const double ar = darea[d];
      ignored = ar < lo || ar > hi;
    }
    if (lane == 0) {
      if (match >= 0) atomicOr(&rec[d].matched, 1ull << bit);
      if (ignored) atomicOr(&rec[d].ignore, 1ull << bit);
    }
  }
}

struct ImageWs {
  size_t zeroed, zeroed_end;        // arena marks around cat_count and area_i: cleared by one memset
  int *cat_count, *area_i;
  double4* dbox;
  double* darea;
  int *rank, *det_of;
  u64* dwords;
  double* ious;
};

ImageWs carve_image(Arena& a, int n, int G, int K, long W64, int max_det) {
  const size_t d = n > 0 ? n : 0, g = G > 0 ? G : 0, k = K > 0 ? K : 0, w64 = W64 > 0 ? W64 : 0;
  a.pad_empty = true;
  ImageWs w;
  w.zeroed = a.mark();
  w.cat_count = a.take<int>(k);
  w.area_i = a.take<int>(d);
  w.zeroed_end = a.mark();
  w.dbox = a.take<double4>(d);
  w.darea = a.take<double>(d);
  w.rank = a.take<int>(d);
  w.det_of = a.take<int>(k * (size_t)(max_det > 0 ? max_det : 0));
  w.dwords = a.take<u64>(d * w64);
  w.ious = a.take<double>(d * g);
  return w;
}

// ----------------------------------------------------------------------------------------------------- accumulate
__global__ __launch_bounds__(256) void coco_key_kernel(const Record* __restrict__ rec, int D, int K, int N,
                                                       int image_bits, u64* __restrict__ key, int* __restrict__ iota) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  const Record r = rec[d];
  int c = r.cat, im = r.image, rk = r.rank;
  if (c < 0 || c >= K || im < 0 || im >= N || rk < 0 || rk >= kMaxDet) { c = K; im = 0; rk = 0; }
  const u32 s = ~float_order_bits(r.score + 0.0f);                     // (-0 + 0 = +0: the two zeros compare equal)
  key[d] = ((u64)c << (32 + image_bits + kRankBits)) | ((u64)s << (image_bits + kRankBits)) | ((u64)im << kRankBits) |
           (u64)rk;
  iota[d] = d;
}

// One workgroup per (category, area range, maxDet).
__global__ __launch_bounds__(kChunk) void coco_pr_kernel(const Record* __restrict__ rec, const int* __restrict__ idx,
                                                         const int* __restrict__ start,
                                                         const long long* __restrict__ npos_table,
                                                         const double* __restrict__ rec_thrs, int R,
                                                         const int* __restrict__ max_dets, int M, int K,
                                                         double* __restrict__ precision, double* __restrict__ scores,
                                                         double* __restrict__ recall) {
  typedef RankedWalk<kChunk> Walk;                 // (eval_walk.h)
  typedef hipcub::BlockScan<int, kChunk> IntScan;
  typedef hipcub::BlockReduce<u64, kChunk> ReduceU;
  __shared__ union {
    typename Walk::Temp walk;
    typename IntScan::TempStorage cnt;
    typename ReduceU::TempStorage redu;
  } temp;
  __shared__ double sh_thr[kMaxR];
  __shared__ typename Walk::Shared sh;
  __shared__ u64 sh_tot[kT + 1];
  const int c = blockIdx.x, a = blockIdx.y, m = blockIdx.z, tid = threadIdx.x;
  const int base = start[c], n = start[c + 1] - base;
  const long long np = npos_table[c * kA + a];
  const int max_det = max_dets[m];
  const long cell = ((long)c * kA + a) * M + m, stride = (long)K * kA * M;   // precision[(t R + r) stride + cell]
  if (np == 0) {                                                         // (block-uniform)
    for (int i = tid; i < kT * R; i += kChunk) { precision[(long)i * stride + cell] = -1.0; scores[(long)i * stride + cell] = -1.0; }
    if (tid < kT) recall[(long)tid * stride + cell] = -1.0;
    return;
  }
  for (int r = tid; r < R; r += kChunk) sh_thr[r] = rec_thrs[r];
  const double npd = (double)np;
  const int nchunk = (n + kChunk - 1) / kChunk;
  const int shift = a * kT;

  // tp in the high word, fp in the low word of threshold t's packed sum
  auto bits_of = [&](u64 mt, u64 ig, int t) -> u64 {
    const u64 mb = (mt >> (shift + t)) & 1ull, ib = (ig >> (shift + t)) & 1ull;
    return ((mb & (ib ^ 1ull)) << 32) | ((mb ^ 1ull) & (ib ^ 1ull));
  };

  // pass 1: the totals per threshold and the number of records within max_det
  u64 mine[kT + 1];
#pragma unroll
  for (int t = 0; t <= kT; ++t) mine[t] = 0;
  for (int k = tid; k < n; k += kChunk) {
    const Record r = rec[idx[base + k]];
    if (r.rank < max_det) {
#pragma unroll
      for (int t = 0; t < kT; ++t) mine[t] += bits_of(r.matched, r.ignore, t);
      mine[kT] += 1;
    }
  }
#pragma unroll
  for (int t = 0; t <= kT; ++t) {
    const u64 tot = ReduceU(temp.redu).Sum(mine[t]);
    if (tid == 0) sh_tot[t] = tot;
    __syncthreads();
  }
  u64 end[kT];                          // running sums at the end of the current chunk
  double env_carry[kT];                 // the envelope right of the current chunk
#pragma unroll
  for (int t = 0; t < kT; ++t) { end[t] = sh_tot[t]; env_carry[t] = 0.0; }
  int end_valid = (int)sh_tot[kT];
  const int nvalid = end_valid;

  // the recall thresholds nobody reaches, and recall itself
#pragma unroll
  for (int t = 0; t < kT; ++t) {
    const double last = (double)(long long)(end[t] >> 32) / npd;
    for (int r = tid; r < R; r += kChunk)
      if (nvalid == 0 || sh_thr[r] > last) {
        precision[((long)t * R + r) * stride + cell] = 0.0;
        scores[((long)t * R + r) * stride + cell] = 0.0;
      }
    if (tid == 0) recall[(long)t * stride + cell] = nvalid ? last : 0.0;
  }

  // pass 2: the chunks from the right
  for (int ch = nchunk - 1; ch >= 0; --ch) {
    const int k = ch * kChunk + tid;
    Record r;
    r.rank = INT_MAX; r.matched = 0; r.ignore = 0; r.score = 0.0f;
    if (k < n) r = rec[idx[base + k]];
    const bool valid = k < n && r.rank < max_det;
    int vinc;
    IntScan(temp.cnt).InclusiveSum(valid ? 1 : 0, vinc);
    if (tid == kChunk - 1) sh.u = (u64)vinc;
    __syncthreads();
    const int begin_valid = end_valid - (int)sh.u;
    const int before = begin_valid + vinc - (valid ? 1 : 0);            // records within max_det in front of this one
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kT; ++t) {
      const u64 b = valid ? bits_of(r.matched, r.ignore, t) : 0ull;
      const u64 inc = Walk::running_sum(temp.walk, sh, b, end[t]);   // (one barrier; end[t] is now the chunk's begin)
      const long long tpc = (long long)(inc >> 32), fpc = (long long)(inc & 0xffffffffull);
      const double rc = (double)tpc / npd;
      const double prec = (valid && tpc + fpc > 0) ? (double)tpc / (double)(tpc + fpc) : 0.0;
      const double env = Walk::envelope(temp.walk, sh, prec, env_carry[t]);     // (two barriers)
      const bool tpbit = (b >> 32) != 0;
      if (valid && (tpbit || before == 0)) {
        // the first record whose recall reaches thr: the one in front of it (if any) is still below
        const double prev = (double)(tpc - (tpbit ? 1 : 0)) / npd;
        const double sc = (double)r.score;
        for (int q = 0; q < R; ++q) {
          const double thr = sh_thr[q];
          if (rc >= thr && (before == 0 || prev < thr)) {
            precision[((long)t * R + q) * stride + cell] = env;
            scores[((long)t * R + q) * stride + cell] = sc;
          }
        }
      }
      __syncthreads();                    // temp and sh are free for the next threshold
    }
    end_valid = begin_valid;
  }
}

struct AccWs {
  int* start;
  u64 *key_a, *key_b;
  int *iota, *idx;
  char* cub;
  size_t cub_bytes;
};

AccWs carve_acc(Arena& a, int D, int K) {
  const size_t d = D > 0 ? D : 0, k = K > 0 ? K : 0;
  a.pad_empty = true;
  AccWs w;
  w.start = a.take<int>(k + 2);
  w.key_a = a.take<u64>(d);
  w.key_b = a.take<u64>(d);
  w.iota = a.take<int>(d);
  w.idx = a.take<int>(d);
  w.cub_bytes = D > 0 ? sort_pairs_temp_bytes(D) : 0;
  w.cub = a.take<char>(w.cub_bytes);
  return w;
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" size_t jtsm_coco_image_workspace_bytes(int n, int G, int K, int H, int W, int max_det) {
  if (n < 0 || G < 0 || K < 1 || H < 0 || W < 0 || max_det < 1 || max_det > kMaxDet) return 0;
  Arena a{nullptr};
  carve_image(a, n, G, K, ((long)H * W + 63) / 64, max_det);
  return a.off;
}

// The keypoints task's own arguments; P == 0: bbox or segm.
struct KeypointArgs {
  const float* det;                 // (n, P, 3)
  const double* gt;                 // (G, P, 3)
  const uint8_t* gt_ignore;         // (G)
  const double* sigmas;             // (P)
  int P;
};

static int coco_image_run(const float* det_boxes, const float* det_scores, const int32_t* det_classes,
                          const uint8_t* det_masks, int n, int H, int W, const double* gt_boxes,
                          const double* gt_area, const uint8_t* gt_crowd, const int32_t* gt_cat_start,
                          const uint64_t* gt_masks, int G, int K, int image_index, int max_det,
                          const double* iou_thrs, const double* area_rng, int64_t* records, int64_t* npos,
                          int64_t* stats, double* ious_debug, int32_t* rank_debug, void* workspace,
                          size_t workspace_bytes, void* stream, const KeypointArgs& kp) {
  JTSM_REQUIRE(n >= 0 && G >= 0 && K >= 1 && H >= 0 && W >= 0 && image_index >= 0,
               "coco_image: n=%d G=%d K=%d H=%d W=%d image_index=%d", n, G, K, H, W, image_index);
  JTSM_REQUIRE(max_det >= 1 && max_det <= kMaxDet, "coco_image: max_det=%d exceeds the %d rank bits of the sort keys "
               "(at most %d)", max_det, kRankBits, kMaxDet);
  JTSM_REQUIRE(n <= 65535, "coco_image: n=%d detections in one image (at most 65535)", n);
  JTSM_REQUIRE(G <= 64 * kMaxGtChunks, "coco_image: G=%d ground-truth objects in one image exceed the %d matched bits "
               "of a lane (at most %d)", G, kMaxGtChunks, 64 * kMaxGtChunks);
  JTSM_REQUIRE((long)n * G <= (1L << 28), "coco_image: n x G = %ld pairs (at most 2^28)", (long)n * G);
  JTSM_REQUIRE(gt_cat_start && iou_thrs && area_rng && npos && stats, "coco_image: null gt_cat_start / params / totals");
  JTSM_REQUIRE(n == 0 || (det_boxes && det_scores && det_classes && records), "coco_image: null detections / records");
  JTSM_REQUIRE(G == 0 || (gt_boxes && gt_area && gt_crowd), "coco_image: null ground truth");
  JTSM_REQUIRE(((size_t)det_boxes & 15) == 0 && ((size_t)gt_boxes & 31) == 0 && ((size_t)records & 7) == 0 &&
                   ((size_t)gt_masks & 7) == 0,
               "coco_image: det_boxes 16-byte, gt_boxes 32-byte, records / gt_masks 8-byte aligned");
  const bool segm = det_masks != nullptr || gt_masks != nullptr;
  const long HW = (long)H * W, W64 = (HW + 63) / 64;
  if (segm) {
    JTSM_REQUIRE(HW >= 1 && HW <= INT_MAX, "coco_image: masks of %d x %d", H, W);
    JTSM_REQUIRE((n == 0 || det_masks) && (G == 0 || gt_masks), "coco_image: segm needs det_masks and gt_masks");
  }
  Arena arena{static_cast<char*>(workspace)};
  const ImageWs w = carve_image(arena, n, G, K, segm ? W64 : 0, max_det);
  JTSM_REQUIRE(workspace && workspace_bytes >= arena.off && ((size_t)workspace & 255) == 0,
               "coco_image: workspace of %zu bytes (256-byte aligned) needed", arena.off);
  hipStream_t st = as_stream(stream);
  int* rank = rank_debug ? rank_debug : w.rank;
  double* ious = ious_debug ? ious_debug : w.ious;
  Record* rec = reinterpret_cast<Record*>(records);

  JTSM_CHECK_HIP(hipMemsetAsync(arena.base + w.zeroed, 0, w.zeroed_end - w.zeroed, st));
  if (n > 0) {
    hipLaunchKernelGGL(coco_rank_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st,
                       reinterpret_cast<const float4*>(det_boxes), det_scores, det_classes, n, K, image_index, max_det,
                       segm ? 1 : 0, w.dbox, w.darea, rank, w.cat_count, w.det_of, rec, reinterpret_cast<u64*>(stats));
    JTSM_CHECK_LAUNCH("coco rank");
    if (segm) {
      const long per_mask = (W64 + 3) / 4;
      hipLaunchKernelGGL(coco_pack_kernel, dim3((unsigned)(per_mask < 64 ? per_mask : 64), n), dim3(256), 0, st,
                         det_masks, HW, W64, w.dwords, w.area_i);
      JTSM_CHECK_LAUNCH("coco pack");
      hipLaunchKernelGGL(coco_area_to_double_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, w.area_i, n, w.darea);
      JTSM_CHECK_LAUNCH("coco area");
    }
    if (G > 0) {
      if (segm) {
        hipLaunchKernelGGL(coco_mask_iou_kernel, dim3(G, n), dim3(256), 0, st, w.dwords, w.area_i, det_classes, rank,
                           reinterpret_cast<const u64*>(gt_masks), gt_crowd, gt_cat_start, K, G, W64, ious);
        JTSM_CHECK_LAUNCH("coco mask iou");
      } else if (kp.P > 0) {
        hipLaunchKernelGGL(coco_oks_kernel, dim3(ceil_div((long)n * G, 256)), dim3(256), 0, st, kp.det, det_classes,
                           rank, n, reinterpret_cast<const double4*>(gt_boxes), gt_area, kp.gt, kp.sigmas, kp.P,
                           gt_cat_start, K, G, ious);
        JTSM_CHECK_LAUNCH("coco oks");
      } else {
        hipLaunchKernelGGL(coco_box_iou_kernel, dim3(ceil_div((long)n * G, 256)), dim3(256), 0, st, w.dbox, det_classes,
                           rank, n, reinterpret_cast<const double4*>(gt_boxes), gt_crowd, gt_cat_start, K, G, ious);
        JTSM_CHECK_LAUNCH("coco box iou");
      }
    }
  }
  hipLaunchKernelGGL(coco_match_kernel, dim3(ceil_div((long)K * kA * kT, 4)), dim3(256), 0, st, w.cat_count, w.det_of,
                     w.darea, n, max_det, gt_area, kp.P > 0 ? kp.gt_ignore : gt_crowd, gt_crowd, gt_cat_start, K, G,
                     ious, iou_thrs, area_rng, rec, reinterpret_cast<u64*>(npos));
  JTSM_CHECK_LAUNCH("coco match");
  return JTSM_OK;
}

extern "C" int jtsm_coco_image(const float* det_boxes, const float* det_scores, const int32_t* det_classes,
                               const uint8_t* det_masks, int n, int H, int W, const double* gt_boxes,
                               const double* gt_area, const uint8_t* gt_crowd, const int32_t* gt_cat_start,
                               const uint64_t* gt_masks, int G, int K, int image_index, int max_det,
                               const double* iou_thrs, const double* area_rng, int64_t* records, int64_t* npos,
                               int64_t* stats, double* ious_debug, int32_t* rank_debug, void* workspace,
                               size_t workspace_bytes, void* stream) {
  return coco_image_run(det_boxes, det_scores, det_classes, det_masks, n, H, W, gt_boxes, gt_area, gt_crowd,
                        gt_cat_start, gt_masks, G, K, image_index, max_det, iou_thrs, area_rng, records, npos, stats,
                        ious_debug, rank_debug, workspace, workspace_bytes, stream, KeypointArgs{});
}

extern "C" size_t jtsm_coco_image_keypoints_workspace_bytes(int n, int G, int K, int P, int max_det) {
  if (P < 1 || P > kMaxKeypoints) return 0;
  return jtsm_coco_image_workspace_bytes(n, G, K, 0, 0, max_det);
}

extern "C" int jtsm_coco_image_keypoints(const float* det_boxes, const float* det_scores, const int32_t* det_classes,
                                         const float* det_keypoints, int n, int P, const double* gt_boxes,
                                         const double* gt_area, const uint8_t* gt_crowd, const uint8_t* gt_ignore,
                                         const double* gt_keypoints, const int32_t* gt_cat_start, int G, int K,
                                         const double* sigmas, int image_index, int max_det, const double* iou_thrs,
                                         const double* area_rng, int64_t* records, int64_t* npos, int64_t* stats,
                                         double* ious_debug, int32_t* rank_debug, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  JTSM_REQUIRE(P >= 1 && P <= kMaxKeypoints, "coco_image_keypoints: P=%d keypoints (1 to %d)", P, kMaxKeypoints);
  JTSM_REQUIRE(sigmas, "coco_image_keypoints: null sigmas");
  JTSM_REQUIRE((n <= 0 || det_keypoints) && (G <= 0 || (gt_keypoints && gt_ignore)),
               "coco_image_keypoints: null det_keypoints / gt_keypoints / gt_ignore");
  JTSM_REQUIRE(((size_t)det_keypoints & 3) == 0 && ((size_t)gt_keypoints & 7) == 0 && ((size_t)sigmas & 7) == 0,
               "coco_image_keypoints: det_keypoints 4-byte, gt_keypoints / sigmas 8-byte aligned");
  return coco_image_run(det_boxes, det_scores, det_classes, nullptr, n, 0, 0, gt_boxes, gt_area, gt_crowd, gt_cat_start,
                        nullptr, G, K, image_index, max_det, iou_thrs, area_rng, records, npos, stats, ious_debug,
                        rank_debug, workspace, workspace_bytes, stream,
                        KeypointArgs{det_keypoints, gt_keypoints, gt_ignore, sigmas, P});
}

extern "C" size_t jtsm_coco_accumulate_workspace_bytes(int D, int K) {
  Arena a{nullptr};
  carve_acc(a, D, K);
  return a.off;
}

extern "C" int jtsm_coco_accumulate(const int64_t* records, int D, int K, int N, const int64_t* npos,
                                    const double* rec_thrs, int R, const int32_t* max_dets, int M, double* precision,
                                    double* scores, double* recall, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  JTSM_REQUIRE(D >= 0 && K >= 1 && N >= 1 && R >= 1 && R <= kMaxR && M >= 1 && M <= kMaxM,
               "coco_accumulate: D=%d K=%d N=%d R=%d (at most %d) M=%d (at most %d)", D, K, N, R, kMaxR, M, kMaxM);
  JTSM_REQUIRE(K <= 65535, "coco_accumulate: K=%d categories (at most 65535)", K);
  const int image_bits = bits_for(N - 1), class_bits = bits_for(K);
  JTSM_REQUIRE(class_bits + 32 + image_bits + kRankBits <= 64,
               "coco_accumulate: K=%d and N=%d need %d + %d bits; the sort key has %d beside the score and the rank", K,
               N, class_bits, image_bits, 64 - 32 - kRankBits);
  JTSM_REQUIRE(npos && rec_thrs && max_dets && precision && scores && recall, "coco_accumulate: null table");
  JTSM_REQUIRE(D == 0 || records, "coco_accumulate: null records");
  JTSM_REQUIRE(((size_t)records & 7) == 0, "coco_accumulate: records must be 8-byte aligned");
  Arena arena{static_cast<char*>(workspace)};
  const AccWs w = carve_acc(arena, D, K);
  JTSM_REQUIRE(workspace && workspace_bytes >= arena.off && ((size_t)workspace & 255) == 0,
               "coco_accumulate: workspace of %zu bytes (256-byte aligned) needed", arena.off);
  hipStream_t st = as_stream(stream);
  const Record* rec = reinterpret_cast<const Record*>(records);
  const int shift = 32 + image_bits + kRankBits;
  if (D > 0) {
    hipLaunchKernelGGL(coco_key_kernel, dim3(ceil_div(D, 256)), dim3(256), 0, st, rec, D, K, N, image_bits, w.key_a,
                       w.iota);
    JTSM_CHECK_LAUNCH("coco key");
    size_t cub_bytes = w.cub_bytes;
    JTSM_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(w.cub, cub_bytes, w.key_a, w.key_b, w.iota, w.idx, D, 0,
                                                      shift + class_bits, st));
  }
  hipLaunchKernelGGL(segment_starts_kernel, dim3(ceil_div(K + 1, 64)), dim3(64), 0, st, w.key_b, D, K, shift, w.start);
  JTSM_CHECK_LAUNCH("coco start");
  hipLaunchKernelGGL(coco_pr_kernel, dim3(K, kA, M), dim3(kChunk), 0, st, rec, w.idx, w.start,
                     reinterpret_cast<const long long*>(npos), rec_thrs, R, max_dets, M, K, precision, scores, recall);
  JTSM_CHECK_LAUNCH("coco pr");
  return JTSM_OK;
}
