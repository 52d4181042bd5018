// C-MIL's two operators for gfx950, for all images of the step at once and without a value read back to the host.
//
// Replaces
//   ROIMerge_forward_cpu / ROIMerge_backward_cpu   projects/WSL/wsl/layers/csrc/ROIMerge/ROIMerge_cpu.cpp:33-232, :234-287
//   ROILabel_forward_cpu                           projects/WSL/wsl/layers/csrc/ROILabel/ROILabel_cpu.cpp:16-194
// which the reference has as host code only (the *_cuda entry points are AT_ERROR): a step copies C, D, the scores and
// an R x R IoU matrix to the host once for the merge and once more per refinement branch for the labelling.  Here the
// IoU is box_iou (box_math.h: pairwise_iou's expression) evaluated where it is needed; no R x R matrix exists.
//
// ROIMerge, per image with n rows (rows [off[b], off[b+1]) of every per-row array):
//   order the rows by S descending, equal S by lower row; top = min(n, 200)
//   for rank t < top, unassigned: it seeds clique cur_id; the ranks tt of [t, min(t + 40, top)), in order, join when
//     unassigned and NOT (IoU(tt, m) < lam) for every member m so far (:134 rejects on `J < lambda`); cur_id += 1
//   every row left becomes its own clique, in row order
//   IC[id] = members; MC[id] = sum over the members n, ascending, of C[n] / IC[id] (each quotient rounded); MD likewise
//   backward: dC[n] = gMC[I[n]] / IC[I[n]]
// The cliques of all images are written compacted: image b's clique `id` is merged row merged_offsets[b] + id, I holds
// merged rows, IC is indexed by merged row, and rows behind merged_offsets[B] are dead (MC = MD = 0, IC = 0).
//
// Five launches, any n:
//   merge_rank    a row's rank is the number of keys above its own (order_key, common.h), counted through LDS tiles of
//                 1024 keys, one thread per row, as many workgroups as the image needs.  Ranks < 200 are kept.
//   merge_walk    ONE WAVEFRONT PER IMAGE.  First, in parallel, for every kept rank a the bit mask back[a]: bit d set
//                 when rank a may share a clique with rank a - d (d < 40): at most 200 x 39 IoUs, 122 per lane.  The
//                 greedy walk is then scalar bit arithmetic: lane = window slot (40 <= 64) holding its rank's mask,
//                 the clique a uniform 64-bit mask M, one candidate slot s per step (the set bits of a ballot of the
//                 unassigned slots): its mask is read from lane s, M reversed and shifted names the distances d at
//                 which members sit, and the candidate joins when its mask has all of them.  Ends with the kept rows
//                 in ascending row order.
//   merge_assign  one thread per row: I, and merged_offsets.
//   merge_means   one thread per (row, class): a row outside the top is its clique; of a top clique the lowest row adds
//                 the members' quotients in ascending row order.
//   merge_backward  elementwise.
//
// ROILabel, per image (one workgroup of 1024):
//   seeds: for each present class ascending, top_k times, the row of largest class score (first maximum; a score must
//     exceed -FLT_MAX, :91-94) among the rows no seed holds yet; when the rows have run out the class gets no seed
//     (the reference would index row -1)
//   match: every row takes the seed of largest IoU (first maximum), w = CW[class of the seed] (the seed's score without CW)
//   assign, in the order perm gives: IoU >= fg and at most num_pos positives so far -> the seed's class, w;
//     else bg_lo <= IoU < bg_hi and at most num_neg negatives so far -> num_classes, w; else the seed's class, 0.
//     With fg >= bg_hi (required) an overflowed positive can never be a negative, so the two caps are two independent
//     exclusive prefix counts along perm: ballots and a running total per 1024 positions.
//   The score is class_score (mining_common.h): mine_top1's.
// No atomics anywhere: the same inputs give the same outputs on every run.
#include <cfloat>

#include "mining_common.h"
#include "reduce.h"
#include "workspace.h"

namespace jtsm {
namespace {

#pragma clang fp contract(off)

typedef unsigned long long u64;

constexpr int kTop = 200;        // ROIMerge_cpu.cpp:105
constexpr int kWindow = 40;      // :116
constexpr int kThreads = 1024;
constexpr int kMaxSeeds = 256;   // present classes x top_k of one image (LDS: 6 KiB)

struct Bag { int off, n, top; };
__device__ __forceinline__ Bag bag_of(const int* __restrict__ bag_off, int b) {
  Bag g;
  g.off = bag_off[b];
  g.n = max(bag_off[b + 1] - g.off, 0);
  g.top = min(g.n, kTop);
  return g;
}

// ---- ROIMerge ----------------------------------------------------------------------------------------------------------
// slot (R): a row's rank when it is < 200, else -1; top_row (B, 200): the row (within the image) of every kept rank.
__global__ __launch_bounds__(kThreads) void merge_rank_kernel(const float* __restrict__ S, const int* __restrict__ bag_off,
                                                              int* __restrict__ slot, int* __restrict__ top_row) {
  __shared__ u64 tile[kThreads];
  const int b = blockIdx.y;
  const Bag g = bag_of(bag_off, b);
  // (the grid is sized from the caller's max_bag_rows; the stride makes every row covered whatever it was)
  for (int base = blockIdx.x * kThreads; base < g.n; base += gridDim.x * kThreads) {   // (uniform)
    const int i = base + threadIdx.x;
    const u64 key[1] = {i < g.n ? order_key(S[g.off + i], i) : ~0ull};   // nothing precedes a padding key
    int before[1];
    count_before<1, kThreads, kThreads, 8>(g.n, [&](int j) { return order_key(S[g.off + j], j); }, key, 1, before, tile);
    if (i < g.n) {
      const bool kept = before[0] < kTop;
      slot[g.off + i] = kept ? before[0] : -1;
      if (kept) top_row[b * kTop + before[0]] = i;
    }
  }
}

// rank_id (B, 200): the clique of every kept rank; sorted_row / sorted_id (B, 200): the kept rows in ascending row order
// with their cliques; num_top (B): cliques among the kept ranks.
__global__ __launch_bounds__(64) void merge_walk_kernel(const float* __restrict__ boxes, const int* __restrict__ bag_off,
                                                        const int* __restrict__ top_row, float lam,
                                                        int* __restrict__ rank_id, int* __restrict__ sorted_row,
                                                        int* __restrict__ sorted_id, int* __restrict__ num_top) {
  __shared__ float4 box[kTop];
  __shared__ u64 back[kTop];
  __shared__ int id[kTop], row[kTop];
  const int b = blockIdx.x, lane = threadIdx.x;
  const Bag g = bag_of(bag_off, b);
  for (int t = lane; t < g.top; t += 64) {
    const int r = top_row[b * kTop + t];
    row[t] = r;
    box[t] = load_box(boxes, (long)g.off + r);
    id[t] = -1;
  }
  __syncthreads();
  for (int a = lane; a < g.top; a += 64) {
    const float4 ba = box[a];
    u64 m = 0;
    for (int d = 1; d < kWindow && a - d >= 0; ++d)
      if (!(box_iou(ba, box[a - d]) < lam)) m |= 1ull << d;   // J[i][j], i the candidate, j the member (:134)
    back[a] = m;
  }
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < g.top; ++t) {
    if (id[t] != -1) continue;                          // (uniform: every lane reads the same word)
    const int end = min(t + kWindow, g.top), r = t + lane;
    const bool valid = r < end;
    const bool open = valid && lane > 0 && id[r] == -1;
    const u64 mine = valid ? back[r] : 0ull;
    const int lo = (int)(unsigned)(mine & 0xffffffffull), hi = (int)(unsigned)(mine >> 32);
    u64 M = 1ull;                                       // the seed; bit k: slot k is a member (uniform)
    for (u64 rest = __ballot(open); rest; rest &= rest - 1ull) {
      const int s = __builtin_amdgcn_readfirstlane(__builtin_ctzll(rest));   // candidate slot, ascending: rank order
      const u64 ok = ((u64)(unsigned)__builtin_amdgcn_readlane(hi, s) << 32) | (unsigned)__builtin_amdgcn_readlane(lo, s);
      const u64 need = __brevll(M) >> (63 - s);         // bit d: the slot s - d is a member (members sit below s)
      if ((need & ~ok) == 0ull) M |= 1ull << s;
    }
    if ((M >> lane) & 1ull) id[r] = cur;                // (bits of M are valid slots only)
    ++cur;
    __syncthreads();
  }
  for (int t = lane; t < g.top; t += 64) {
    const int r = row[t];
    int pos = 0;
    for (int u = 0; u < g.top; ++u) pos += row[u] < r ? 1 : 0;
    rank_id[b * kTop + t] = id[t];
    sorted_row[b * kTop + pos] = r;
    sorted_id[b * kTop + pos] = id[t];
  }
  if (lane == 0) num_top[b] = cur;
}

__device__ __forceinline__ int merged_count(const int* __restrict__ bag_off, const int* __restrict__ num_top, int b) {
  const Bag g = bag_of(bag_off, b);
  return num_top[b] + g.n - g.top;
}

__global__ __launch_bounds__(256) void merge_assign_kernel(const int* __restrict__ bag_off, int B, int R,
                                                           const int* __restrict__ slot, const int* __restrict__ rank_id,
                                                           const int* __restrict__ sorted_row,
                                                           const int* __restrict__ num_top, int* __restrict__ I,
                                                           int* __restrict__ merged_off) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  if (r == 0) {
    int acc = 0;
    merged_off[0] = 0;
    for (int b = 0; b < B; ++b) { acc += merged_count(bag_off, num_top, b); merged_off[b + 1] = acc; }
  }
  const int img = image_of(bag_off, B, r);
  const Bag g = bag_of(bag_off, img);
  int base = 0;
  for (int b = 0; b < img; ++b) base += merged_count(bag_off, num_top, b);
  const int s = slot[r], local = r - g.off;
  int lid;
  if (s >= 0) {
    lid = rank_id[img * kTop + s];
  } else {                                              // its own clique, after the top's, in row order
    int kept_below = 0;
    for (int j = 0; j < g.top; ++j) kept_below += sorted_row[img * kTop + j] < local ? 1 : 0;
    lid = num_top[img] + local - kept_below;
  }
  I[r] = base + lid;
}

// Every live merged row is written by the thread of its lowest member, every dead row (>= merged_off[B]) zeroed by
// the thread of the same index: no row is written twice.
__global__ __launch_bounds__(256) void merge_means_kernel(const float* __restrict__ C, int ldc, const float* __restrict__ D,
                                                          int ldd, int K, const int* __restrict__ bag_off, int B, int R,
                                                          const int* __restrict__ slot, const int* __restrict__ rank_id,
                                                          const int* __restrict__ sorted_row,
                                                          const int* __restrict__ sorted_id, const int* __restrict__ I,
                                                          const int* __restrict__ merged_off, float* __restrict__ MC,
                                                          float* __restrict__ MD, int* __restrict__ IC) {
#pragma clang fp contract(off)
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)R * K) return;
  const int r = (int)(idx / K), c = (int)(idx - (long)r * K);
  if (r >= merged_off[B]) {                             // a dead row
    MC[(size_t)r * K + c] = 0.f;
    MD[(size_t)r * K + c] = 0.f;
    if (c == 0) IC[r] = 0;
  }
  const int img = image_of(bag_off, B, r);
  const Bag g = bag_of(bag_off, img);
  const int s = slot[r];
  const size_t m = (size_t)I[r];
  int cnt = 1, first = r - g.off, lid = -1;
  const int* __restrict__ srow = sorted_row + img * kTop;
  const int* __restrict__ sid = sorted_id + img * kTop;
  if (s >= 0) {
    lid = rank_id[img * kTop + s];
    cnt = 0;
    first = -1;
    for (int j = 0; j < g.top; ++j)
      if (sid[j] == lid) { if (first < 0) first = srow[j]; ++cnt; }
    if (first != r - g.off) return;                     // the clique's lowest row adds for it
  }
  const float fc = (float)cnt;
  float ac = 0.f, ad = 0.f;                             // (the reference adds into zeros)
  if (s < 0) {
    ac += C[(size_t)r * ldc + c] / fc;
    ad += D[(size_t)r * ldd + c] / fc;
  } else {
    for (int j = 0; j < g.top; ++j)
      if (sid[j] == lid) {
        const size_t n = (size_t)(g.off + srow[j]);
        ac += C[n * ldc + c] / fc;
        ad += D[n * ldd + c] / fc;
      }
  }
  MC[m * K + c] = ac;
  MD[m * K + c] = ad;
  if (c == 0) IC[m] = cnt;
}

__global__ __launch_bounds__(256) void merge_backward_kernel(const float* __restrict__ gMC, const float* __restrict__ gMD,
                                                             int ldg, int K, const int* __restrict__ I,
                                                             const int* __restrict__ IC, int R, float* __restrict__ dC,
                                                             float* __restrict__ dD, int ld_grad) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)R * K) return;
  const int r = (int)(idx / K), c = (int)(idx - (long)r * K);
  const size_t m = (size_t)I[r];
  const float fc = (float)IC[m];
  dC[(size_t)r * ld_grad + c] = gMC[m * ldg + c] / fc;
  dD[(size_t)r * ld_grad + c] = gMD[m * ldg + c] / fc;
}

struct MergeWs { int* slot; int* top_row; int* rank_id; int* sorted_row; int* sorted_id; int* num_top; };
MergeWs carve(Arena& a, int B, int R) {
  const size_t tab = (size_t)B * kTop;
  MergeWs k;
  k.slot = a.take<int>(R);
  k.top_row = a.take<int>(tab);
  k.rank_id = a.take<int>(tab);
  k.sorted_row = a.take<int>(tab);
  k.sorted_id = a.take<int>(tab);
  k.num_top = a.take<int>(B);
  return k;
}

// ---- ROILabel ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void roi_label_kernel(
    const float* __restrict__ S, int ld, const float* __restrict__ lse, const float* __restrict__ boxes,
    const int* __restrict__ bag_off, const int* __restrict__ classes, const int* __restrict__ counts, int G,
    const float* __restrict__ CW, int ld_cw, const int* __restrict__ perm, float fg, float bg_hi, float bg_lo,
    int num_pos, int num_neg, int top_k, int num_classes, int* __restrict__ labels, float* __restrict__ weights,
    int* __restrict__ seed_rows, int* __restrict__ seed_num) {
  __shared__ float4 s_box[kMaxSeeds];
  __shared__ int s_row[kMaxSeeds], s_cls[kMaxSeeds];
  __shared__ float s_w[kMaxSeeds];
  __shared__ u64 wave_slot[kThreads / 64];
  __shared__ int wave_count[kThreads / 64];
  const int b = blockIdx.x, t = threadIdx.x;
  const Bag g = bag_of(bag_off, b);
  const int c = min(max(counts[b], 0), G);
  const int P = G * top_k;                              // <= kMaxSeeds (the host checks)

  // ---- seeds
  int ns = 0;                                           // (uniform)
  bool out_of_rows = false;
  for (int q = 0; q < c && !out_of_rows; ++q) {
    const int cls = classes[b * G + q];
    for (int k = 0; k < top_k; ++k) {
      float best = -FLT_MAX;
      int at = -1;
      for (int i = t; i < g.n; i += kThreads) {         // ascending rows, strict: the thread's first maximum
        const float v = class_score(S, ld, lse, g.off + i, cls);
        if (best < v) {
          bool taken = false;
          for (int j = 0; j < ns; ++j) taken = taken || s_row[j] == i;
          if (!taken) { best = v; at = i; }
        }
      }
      // (order_key: the lowest row among equal scores)
      const u64 key = wg_reduce<kThreads / 64>(at >= 0 ? order_key(best, at) : 0ull, Max(), wave_slot);
      if (key == 0ull) { out_of_rows = true; break; }   // (uniform)
      const int row = (int)key_index(key);
      if (t == 0) {
        s_row[ns] = row;
        s_cls[ns] = cls;
        s_w[ns] = CW ? CW[(size_t)b * ld_cw + cls] : class_score(S, ld, lse, g.off + row, cls);
        s_box[ns] = load_box(boxes, (long)g.off + row);
      }
      ++ns;
      __syncthreads();
    }
  }
  for (int j = t; j < P; j += kThreads) seed_rows[(size_t)b * P + j] = j < ns ? s_row[j] : -1;
  if (t == 0) seed_num[b] = ns;

  // ---- match and assign, 1024 positions of perm at a time
  int npos = 0, nneg = 0;                               // taken so far (uniform)
  for (int p0 = 0; p0 < g.n; p0 += kThreads) {
    const int p = p0 + t;
    int i = p < g.n ? perm[g.off + p] : -1;
    const bool valid = i >= 0 && i < g.n;               // (a row outside the image is never written)
    float best = -FLT_MAX;
    int at = -1;
    if (valid) {
      const float4 bx = load_box(boxes, (long)g.off + i);
      for (int j = 0; j < ns; ++j) {
        const float v = box_iou(bx, s_box[j]);
        if (best < v) { best = v; at = j; }             // strict: the first maximum
      }
    }
    const bool is_fg = at >= 0 && best >= fg;
    const bool is_bg = at >= 0 && !is_fg && best >= bg_lo && best < bg_hi;
    int cp, cn;
    const int sp = compact_wg<kThreads / 64>(is_fg, wave_count, cp);
    const int sn = compact_wg<kThreads / 64>(is_bg, wave_count, cn);
    if (valid) {
      int label = num_classes;
      float w = 0.f;
      if (at >= 0) {
        label = s_cls[at];
        w = s_w[at];
        if (is_fg && npos + sp <= num_pos) {
        } else if (is_bg && nneg + sn <= num_neg) {
          label = num_classes;
        } else {
          w = 0.f;
        }
      }
      labels[g.off + i] = label;
      weights[g.off + i] = w;
    }
    npos += cp;
    nneg += cn;
  }
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" {

size_t jtsm_roi_merge_workspace_bytes(int B, int R) {
  if (B <= 0 || R < 0) return 256;
  Arena a{nullptr};
  carve(a, B, R);
  return a.off;
}

int jtsm_roi_merge_forward_f32(const float* S, const float* boxes, const float* C, int ldc, const float* D, int ldd,
                               int K, const int32_t* bag_offsets, int B, int R, int max_bag_rows, float lam, float* MC,
                               float* MD, int32_t* I, int32_t* IC, int32_t* merged_offsets, void* workspace,
                               void* stream) {
  JTSM_REQUIRE(B > 0 && B <= 65535 && R >= 0 && K > 0 && ldc >= K && ldd >= K && max_bag_rows >= 0 &&
               (long)B * max_bag_rows >= R, "roi_merge: bad sizes (B %d, R %d, K %d, max_bag_rows %d)", B, R, K,
               max_bag_rows);
  JTSM_REQUIRE(bag_offsets && merged_offsets && workspace, "roi_merge: null pointer");
  hipStream_t st = as_stream(stream);
  if (R == 0) {
    JTSM_CHECK_HIP(hipMemsetAsync(merged_offsets, 0, (size_t)(B + 1) * sizeof(int32_t), st));
    return JTSM_OK;
  }
  JTSM_REQUIRE(S && boxes && C && D && MC && MD && I && IC, "roi_merge: null pointer");
  JTSM_REQUIRE((reinterpret_cast<uintptr_t>(boxes) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
               "roi_merge: boxes must be 16-byte and the workspace 256-byte aligned");
  Arena arena{static_cast<char*>(workspace)};
  const MergeWs k = carve(arena, B, R);
  hipLaunchKernelGGL(merge_rank_kernel, dim3(ceil_div(max_bag_rows, kThreads), B), dim3(kThreads), 0, st, S, bag_offsets,
                     k.slot, k.top_row);
  hipLaunchKernelGGL(merge_walk_kernel, dim3(B), dim3(64), 0, st, boxes, bag_offsets, k.top_row, lam, k.rank_id,
                     k.sorted_row, k.sorted_id, k.num_top);
  hipLaunchKernelGGL(merge_assign_kernel, dim3(ceil_div(R, 256)), dim3(256), 0, st, bag_offsets, B, R, k.slot, k.rank_id,
                     k.sorted_row, k.num_top, I, merged_offsets);
  hipLaunchKernelGGL(merge_means_kernel, dim3(ceil_div((long)R * K, 256)), dim3(256), 0, st, C, ldc, D, ldd, K,
                     bag_offsets, B, R, k.slot, k.rank_id, k.sorted_row, k.sorted_id, I, merged_offsets, MC, MD, IC);
  JTSM_CHECK_LAUNCH("roi_merge");
  return JTSM_OK;
}

int jtsm_roi_merge_backward_f32(const float* gMC, const float* gMD, int ld, int K, const int32_t* I, const int32_t* IC,
                                int R, float* dC, float* dD, int ld_grad, void* stream) {
  JTSM_REQUIRE(R >= 0 && K > 0 && ld >= K && ld_grad >= K, "roi_merge backward: bad sizes");
  if (R == 0) return JTSM_OK;
  JTSM_REQUIRE(gMC && gMD && I && IC && dC && dD, "roi_merge backward: null pointer");
  hipLaunchKernelGGL(merge_backward_kernel, dim3(ceil_div((long)R * K, 256)), dim3(256), 0, as_stream(stream), gMC, gMD,
                     ld, K, I, IC, R, dC, dD, ld_grad);
  JTSM_CHECK_LAUNCH("roi_merge backward");
  return JTSM_OK;
}

int jtsm_roi_label_f32(const float* S, int ld, const float* lse, const float* boxes, const int32_t* bag_offsets,
                       const int32_t* classes, const int32_t* counts, int B, int G, const float* CW, int ld_cw,
                       const int32_t* perm, float fg, float bg_hi, float bg_lo, int num_pos, int num_neg, int top_k,
                       int num_classes, int32_t* labels, float* weights, int32_t* seed_rows, int32_t* seed_num,
                       void* stream) {
  JTSM_REQUIRE(B >= 0 && G >= 0 && top_k > 0 && ld >= 0 && num_classes > 0 && num_pos >= 0 && num_neg >= 0,
               "roi_label: bad sizes (B %d, G %d, top_k %d)", B, G, top_k);
  JTSM_REQUIRE((long)G * top_k <= kMaxSeeds, "roi_label: at most %d seeds per image, got %d classes x top_k %d",
               kMaxSeeds, G, top_k);
  JTSM_REQUIRE(fg >= bg_hi, "roi_label: fg_thresh %g must not be below bg_thresh_hi %g", (double)fg, (double)bg_hi);
  if (B == 0) return JTSM_OK;
  JTSM_REQUIRE(S && boxes && bag_offsets && counts && perm && labels && weights && seed_num && (G == 0 || (classes && seed_rows)),
               "roi_label: null pointer");
  JTSM_REQUIRE(!CW || ld_cw > 0, "roi_label: CW needs its leading dimension");
  JTSM_REQUIRE((reinterpret_cast<uintptr_t>(boxes) & 15) == 0, "roi_label: boxes must be 16-byte aligned");
  hipLaunchKernelGGL(roi_label_kernel, dim3(B), dim3(kThreads), 0, as_stream(stream), S, ld, lse, boxes, bag_offsets,
                     classes, counts, G, CW, ld_cw, perm, fg, bg_hi, bg_lo, num_pos, num_neg, top_k, num_classes, labels,
                     weights, seed_rows, seed_num);
  JTSM_CHECK_LAUNCH("roi_label");
  return JTSM_OK;
}

}  // extern "C"
