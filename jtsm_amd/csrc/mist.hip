// MIST pseudo-ground-truth mining (projects/WSL/wsl/modeling/roi_heads/roi_heads_oicr.py:550-591 get_pgt_mist on
// :660-811 get_pgt_top_k with top_k = top_pro < 1, need_instance = False), for all images of the step at once and
// without a single value read back to the host.
//
// Per image b with n proposals, c = counts[b] present classes and t = min(top_t[b], n):
//   1. per class slot g < c, the t rows with the highest class score, descending, equal scores by ascending row
//      (torch.topk, :730-733); candidate (j, g) has list index j * c + g (the (t, c) tensor flattened, :783-785);
//      its box is mined_box (mining_common.h: mine_top1's);
//   2. one greedy NMS over the t * c candidates as a single class (batched_nms with all-zero idxs, :564-568: the
//      coordinate offset is zero): visited by descending score, equal scores by ascending list index, a candidate is
//      dropped when its IoU with an earlier survivor is > iou_thresh (iou_above: the detections' NMS test);
//   3. the survivors in visiting order, weights = scores (:584-586), padding zero-filled.
//
// Three launches.
//   mist_topk    one workgroup per (image, class slot).  A row's position in the class's descending order is the NUMBER
//                OF ROWS THAT PRECEDE IT — counted, not sorted: 64-bit keys (ordered score bits, ~row) make the order
//                total, the image's keys pass through LDS in tiles of 4096 (broadcast reads), every thread counts for
//                up to 8 rows of its own.  A row whose count is < t is candidate j = count.  Any n: rows beyond
//                8 * 1024 take further passes.
//   mist_rank    the same count over the image's candidates (key: ordered score bits, ~list index), 1024 candidates per
//                workgroup, as many workgroups as the list needs: the candidates in visiting order.
//   mist_nms     one workgroup per image walks the visiting order 1024 candidates at a time.  A chunk is first tested
//                against every survivor so far (all 16 wavefronts in parallel, the survivors read back from the output
//                this workgroup wrote), then its wavefronts take turns, in order: a wavefront settles its 64 candidates
//                among themselves (64 x 64 IoU bits in registers, a ballot of the live lanes, a 64-step scan over
//                shuffled words), appends its survivors to the output and publishes them through LDS to the
//                wavefronts behind it.  There is no per-list state in LDS, so no list is too long for it.
// Nothing depends on the arrival order of atomics: there are none.
#include <cfloat>

#include "mining_common.h"
#include "reduce.h"
#include "workspace.h"

namespace jtsm {
namespace {

typedef unsigned long long u64;

constexpr int kThreads = 1024;
constexpr int kOwn = 8;         // rows a thread counts for in one pass of mist_topk
constexpr int kTile = 4096;     // keys in LDS at a time

// (order_key — score descending, then index ascending: common.h; class_score, mined_box, count_before: mining_common.h)

struct ImageList { int r0, n, c, t, N; };
__device__ __forceinline__ ImageList image_list(const int* __restrict__ bag_off, const int* __restrict__ counts,
                                                const int* __restrict__ top_t, int b, int G, int t_max) {
  ImageList l;
  l.r0 = bag_off[b];
  l.n = max(bag_off[b + 1] - l.r0, 0);
  l.c = min(max(counts[b], 0), G);
  l.t = min(min(max(top_t[b], 0), t_max), l.n);
  l.N = l.t * l.c;                    // <= t_max * G = P
  return l;
}

__global__ __launch_bounds__(kThreads) void mist_topk_kernel(
    const float* __restrict__ scores, int ld, const float* __restrict__ lse, const float* __restrict__ proposals,
    const float* __restrict__ deltas, int ld_d, int decode_zero, const int* __restrict__ bag_off,
    const int* __restrict__ classes, const int* __restrict__ counts, const int* __restrict__ top_t, int G, int t_max,
    int P, float* __restrict__ cand_score, int* __restrict__ cand_row, float4* __restrict__ cand_box) {
  __shared__ u64 tile[kTile];
  const int b = blockIdx.x / G, g = blockIdx.x - b * G;
  const ImageList l = image_list(bag_off, counts, top_t, b, G, t_max);
  if (g >= l.c || l.t == 0) return;                     // (uniform)
  const int cls = classes[b * G + g];
  for (int own0 = 0; own0 < l.n; own0 += kOwn * kThreads) {
    const int own_n = min(kOwn, (l.n - own0 + kThreads - 1) / kThreads);   // (uniform)
    float val[kOwn];
    u64 key[kOwn];
    int before[kOwn];
#pragma unroll
    for (int u = 0; u < kOwn; ++u) {
      const int i = own0 + u * kThreads + (int)threadIdx.x;
      val[u] = (u < own_n && i < l.n) ? class_score(scores, ld, lse, l.r0 + i, cls) : 0.f;
      key[u] = (u < own_n && i < l.n) ? order_key(val[u], i) : ~0ull;   // nothing precedes a padding key
    }
    count_before<kOwn, kTile, kThreads, 0>(l.n, [&](int i) { return order_key(class_score(scores, ld, lse, l.r0 + i, cls), i); }, key,
                                           own_n, before, tile);
#pragma unroll
    for (int u = 0; u < kOwn; ++u) {
      const int i = own0 + u * kThreads + (int)threadIdx.x;
      if (u < own_n && i < l.n && before[u] < l.t) {
        const size_t o = (size_t)b * P + (size_t)before[u] * l.c + g;
        const int r = l.r0 + i;
        cand_score[o] = val[u];
        cand_row[o] = i;
        cand_box[o] = mined_box(proposals, deltas, ld_d, decode_zero, r, cls);
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void mist_rank_kernel(
    const int* __restrict__ bag_off, const int* __restrict__ counts, const int* __restrict__ top_t, int G, int t_max,
    int P, const float* __restrict__ cand_score, const float4* __restrict__ cand_box, float4* __restrict__ sorted_box,
    int* __restrict__ sorted_idx) {
  __shared__ u64 tile[kThreads];
  const int b = blockIdx.y;
  const ImageList l = image_list(bag_off, counts, top_t, b, G, t_max);
  if ((int)blockIdx.x * kThreads >= l.N) return;        // (uniform)
  const float* sc = cand_score + (size_t)b * P;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const u64 key[1] = {i < l.N ? order_key(sc[i], i) : ~0ull};
  int before[1];
  count_before<1, kThreads, kThreads, 0>(l.N, [&](int j) { return order_key(sc[j], j); }, key, 1, before, tile);
  if (i < l.N) {
    sorted_box[(size_t)b * P + before[0]] = cand_box[(size_t)b * P + i];
    sorted_idx[(size_t)b * P + before[0]] = i;
  }
}

// out_box is read back by the workgroup that writes it (behind a barrier): no __restrict__, no const.
__global__ __launch_bounds__(kThreads) void mist_nms_kernel(
    const int* __restrict__ bag_off, const int* __restrict__ classes, const int* __restrict__ counts,
    const int* __restrict__ top_t, int G, int t_max, int P, float thr, const float* __restrict__ cand_score,
    const int* __restrict__ cand_row, const float4* __restrict__ sorted_box, const int* __restrict__ sorted_idx,
    float4* out_box, int* __restrict__ out_cls, float* __restrict__ out_score, float* __restrict__ out_weight,
    int* __restrict__ out_row, int* __restrict__ out_num) {
  __shared__ float4 fresh[64];      // the survivors of the wavefront whose turn it is
  __shared__ int fresh_n;
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const ImageList l = image_list(bag_off, counts, top_t, b, G, t_max);
  const size_t base = (size_t)b * P;
  int K = 0;                        // survivors so far (the same value in every thread)
  for (int p0 = 0; p0 < l.N; p0 += kThreads) {
    const int p = p0 + threadIdx.x;
    const bool valid = p < l.N;
    const float4 box = valid ? sorted_box[base + p] : make_float4(0.f, 0.f, 0.f, 0.f);
    bool live = valid;
    for (int k = 0; k < K; ++k) {
      const float4 kb = out_box[base + k];
      live = live && !iou_above(kb, box, thr);
    }
    for (int s = 0; s < kThreads / 64; ++s) {
      if (wv == s) {                // (wavefront-uniform)
        u64 mine = 0;               // bit j: this lane's box suppresses lane j's (j behind it)
        for (int j = 0; j < 64; ++j) {
          const float4 ob = shfl_box(box, j);
          if (j > lane && iou_above(box, ob, thr)) mine |= 1ull << j;
        }
        u64 gone = ~__ballot(live), kept = 0;
        for (int j = 0; j < 64; ++j) {
          const u64 w = shfl64(mine, j);
          if (!((gone >> j) & 1ull)) { kept |= 1ull << j; gone |= w; }
        }
        const int slot = __popcll(kept & ((1ull << lane) - 1ull));
        if ((kept >> lane) & 1ull) {
          const int i = sorted_idx[base + p];
          const size_t o = base + K + slot;
          const float sc = cand_score[base + i];
          out_box[o] = box;
          out_cls[o] = classes[b * G + i % l.c];
          out_score[o] = sc;
          out_weight[o] = sc;       // gt_weights = pgt_scores (:584-586)
          out_row[o] = cand_row[base + i];
          fresh[slot] = box;
        }
        if (lane == 0) fresh_n = __popcll(kept);
        live = false;               // settled
      }
      __syncthreads();              // (also orders this workgroup's out_box stores before its later loads)
      const int fn = fresh_n;
      if (wv > s && live)
        for (int k = 0; k < fn; ++k) live = live && !iou_above(fresh[k], box, thr);
      K += fn;
      __syncthreads();              // fresh / fresh_n are free for the next wavefront
    }
  }
  for (int k = K + threadIdx.x; k < P; k += kThreads) {
    out_box[base + k] = make_float4(0.f, 0.f, 0.f, 0.f);
    out_cls[base + k] = 0;
    out_score[base + k] = 0.f;
    out_weight[base + k] = 0.f;
    out_row[base + k] = 0;
  }
  if (threadIdx.x == 0) out_num[b] = K;
}

struct MistWs { float* cand_score; int* cand_row; float4* cand_box; float4* sorted_box; int* sorted_idx; };
MistWs carve(Arena& a, int B, int P) {
  const size_t n = (size_t)B * (size_t)P;
  MistWs k;
  k.cand_box = a.take<float4>(n);
  k.sorted_box = a.take<float4>(n);
  k.cand_score = a.take<float>(n);
  k.cand_row = a.take<int>(n);
  k.sorted_idx = a.take<int>(n);
  return k;
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" {

size_t jtsm_mine_top_p_workspace_bytes(int B, int G, int t_max) {
  if (B <= 0 || G <= 0 || t_max <= 0) return 256;
  Arena a{nullptr};
  carve(a, B, G * t_max);
  return a.off;
}

int jtsm_mine_top_p_f32(const float* scores, int ld, const float* lse, const float* proposals, const float* deltas,
                        int ld_deltas, int decode_zero_deltas, const int32_t* bag_offsets, const int32_t* classes,
                        const int32_t* counts, const int32_t* top_t, int B, int G, int t_max, float iou_thresh,
                        float* out_boxes, int32_t* out_classes, float* out_scores, float* out_weights,
                        int32_t* out_rows, int32_t* out_num, void* workspace, void* stream) {
  JTSM_REQUIRE(B >= 0 && G >= 0 && t_max >= 0 && ld >= 0 && (long)G * t_max < (1L << 24) && (long)B * G < (1L << 30),
               "mine_top_p: bad sizes (B %d, G %d, t_max %d)", B, G, t_max);
  if (B == 0) return JTSM_OK;
  JTSM_REQUIRE(bag_offsets && classes && counts && top_t && out_num, "mine_top_p: null pointer");
  hipStream_t st = as_stream(stream);
  const int P = G * t_max;
  if (P == 0) {
    JTSM_CHECK_HIP(hipMemsetAsync(out_num, 0, (size_t)B * sizeof(int32_t), st));
    return JTSM_OK;
  }
  JTSM_REQUIRE(scores && proposals && out_boxes && out_classes && out_scores && out_weights && out_rows && workspace,
               "mine_top_p: null pointer");
  JTSM_REQUIRE(!deltas || ld_deltas >= 4, "mine_top_p: deltas need their leading dimension");
  JTSM_REQUIRE((reinterpret_cast<uintptr_t>(out_boxes) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0,
               "mine_top_p: out_boxes must be 16-byte and the workspace 256-byte aligned");
  Arena arena{static_cast<char*>(workspace)};
  const MistWs k = carve(arena, B, P);
  hipLaunchKernelGGL(mist_topk_kernel, dim3(B * G), dim3(kThreads), 0, st, scores, ld, lse, proposals, deltas, ld_deltas,
                     decode_zero_deltas, bag_offsets, classes, counts, top_t, G, t_max, P, k.cand_score, k.cand_row,
                     k.cand_box);
  hipLaunchKernelGGL(mist_rank_kernel, dim3(ceil_div(P, kThreads), B), dim3(kThreads), 0, st, bag_offsets, counts, top_t,
                     G, t_max, P, k.cand_score, k.cand_box, k.sorted_box, k.sorted_idx);
  hipLaunchKernelGGL(mist_nms_kernel, dim3(B), dim3(kThreads), 0, st, bag_offsets, classes, counts, top_t, G, t_max, P,
                     iou_thresh, k.cand_score, k.cand_row, k.sorted_box, k.sorted_idx,
                     reinterpret_cast<float4*>(out_boxes), out_classes, out_scores, out_weights, out_rows, out_num);
  JTSM_CHECK_LAUNCH("mine_top_p");
  return JTSM_OK;
}

}  // extern "C"
