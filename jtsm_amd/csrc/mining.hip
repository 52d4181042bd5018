// Pseudo-ground-truth mining and proposal labelling of JTSMROIHeads, fused.
//
// Replaces, per refinement round, the chain of ~150 small PyTorch launches (and several host syncs) of
//   get_pgt_top_k            projects/WSL/wsl/modeling/roi_heads/roi_heads_jtsm.py:1167-1338 (top_k = 1)
//   label_and_sample_proposals  projects/WSL/wsl/modeling/roi_heads/roi_heads.py:264-370
//     (pairwise_iou detectron2/structures/boxes.py:345-392, Matcher([0.5],[0,1]) modeling/matcher.py:61-103)
//   predict_probs / predict_boxes  .../fast_rcnn_oicr.py:684-783 (softmax, Box2BoxTransform.apply_deltas
//     detectron2/modeling/box_regression.py:73-113) — evaluated only where they are consumed
// by three launches: row log-sum-exp, one block-wide arg-max per (image, present class), and one
// IoU-match per proposal.  Results are integers (winning rows, labels, matched indices) plus the copied
// pseudo boxes / weights, in exactly the layout the OICR loss kernel takes.
// Floating-point steps that decide integers (IoU, box decoding) are evaluated un-contracted, in the
// reference's operation order.
#include <cfloat>

#include "mining_common.h"
#include "reduce.h"

namespace jtsm {
namespace {

#pragma clang fp contract(off)

// lse[r] = log(sum_c exp(z[r,c]))   (wavefront per row, any ncls)
__global__ __launch_bounds__(256) void row_lse_kernel(const float* __restrict__ z, int ld, int ncls, int R,
                                                      float* __restrict__ lse) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const float* row = z + (size_t)r * ld;
  float mx = -FLT_MAX;
  for (int c = lane; c < ncls; c += 64) mx = fmaxf(mx, row[c]);
  mx = wave_max(mx);
  float sm = 0.f;
  for (int c = lane; c < ncls; c += 64) sm += expf(row[c] - mx);
  sm = wave_sum(sm);
  if (lane == 0) lse[r] = mx + logf(sm);
}

// One workgroup per (image, class slot): arg-max over the image's proposals of the class score
// (class_score); lowest row wins ties.  A NaN is never picked, nor a score that does not exceed -FLT_MAX: an image
// with nothing to pick answers with its first row.
__global__ __launch_bounds__(256) void mine_top1_kernel(const float* __restrict__ scores, int ld,
                                                        const float* __restrict__ lse,
                                                        const float* __restrict__ proposals,
                                                        const float* __restrict__ deltas, int ld_d,
                                                        const int* __restrict__ bag_off,
                                                        const int* __restrict__ classes,
                                                        const int* __restrict__ counts, int Gmax,
                                                        const float* __restrict__ img_probs, int nprob,
                                                        int* __restrict__ out_idx, float* __restrict__ out_box,
                                                        float* __restrict__ out_score,
                                                        float* __restrict__ out_weight) {
  __shared__ BestPair slot[4];
  const int img = blockIdx.x / Gmax, g = blockIdx.x - img * Gmax;
  if (g >= counts[img]) return;
  const int cls = classes[img * Gmax + g];
  const int r0 = bag_off[img], r1 = bag_off[img + 1];
  float best = -FLT_MAX;
  int at = kNoIndex;
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const float v = class_score(scores, ld, lse, r, cls);
    if (v > best) { best = v; at = r; }
  }
  const BestPair top = wg_arg_best<4>(best, at, slot);
  if (threadIdx.x == 0) {
    const int r = best_index(top) == kNoIndex ? r0 : best_index(top);
    const int o = img * Gmax + g;
    out_idx[o] = r - r0;
    out_score[o] = best_value(top);
    out_weight[o] = img_probs[(size_t)img * nprob + cls];
    const float4 bx = mined_box(proposals, deltas, ld_d, 0, r, cls);
    out_box[4 * o] = bx.x; out_box[4 * o + 1] = bx.y; out_box[4 * o + 2] = bx.z; out_box[4 * o + 3] = bx.w;
  }
}

// One thread per proposal: IoU against the image's pseudo boxes, first maximum wins; label = class of
// the best box if IoU >= thresh else bg_label; also copies that box / weight / score.
__global__ __launch_bounds__(256) void match_label_kernel(const float* __restrict__ proposals,
                                                          const int* __restrict__ bag_off, int B, int R,
                                                          const float* __restrict__ pgt_box,
                                                          const int* __restrict__ classes,
                                                          const int* __restrict__ counts,
                                                          const float* __restrict__ pgt_weight,
                                                          const float* __restrict__ pgt_score, int Gmax,
                                                          float thresh, int bg_label, int* __restrict__ labels,
                                                          int* __restrict__ matched, float* __restrict__ gt_boxes,
                                                          float* __restrict__ gt_weights,
                                                          float* __restrict__ gt_scores) {
#pragma clang fp contract(off)
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int img = image_of(bag_off, B, r);
  const float* p = proposals + 4 * (size_t)r;
  const float4 pb = box_at(proposals, r);
  const int n = counts[img];
  float best = -1.f;
  int at = 0;
  for (int g = 0; g < n; ++g) {
    const float iou = box_iou(box_at(pgt_box, (long)img * Gmax + g), pb);   // (target, proposal)
    if (iou > best) { best = iou; at = g; }
  }
  const int o = img * Gmax + at;
  if (n == 0) {
    labels[r] = bg_label;
    matched[r] = 0;
    for (int k = 0; k < 4; ++k) gt_boxes[4 * (size_t)r + k] = p[k];
    gt_weights[r] = 0.f;
    if (gt_scores) gt_scores[r] = 0.f;
    return;
  }
  labels[r] = best >= thresh ? classes[o] : bg_label;
  matched[r] = at;
  for (int k = 0; k < 4; ++k) gt_boxes[4 * (size_t)r + k] = pgt_box[4 * (size_t)o + k];
  gt_weights[r] = pgt_weight[o];
  if (gt_scores) gt_scores[r] = pgt_score[o];
}

// ---- the "10 nearest" targets of the mask branch (roi_heads_jtsm.py:840-905): for every pseudo-GT box, the top_k
// FOREGROUND proposals of its image by IoU with it (torch.topk over pairwise_iou(targets, fg proposals), k = min(#fg,
// top_k)); ordering here: IoU descending, equal IoUs by ascending proposal row.  One workgroup per (image, pseudo box);
// round j picks the smallest key (−IoU, row) greater than round j-1's.  near_rows (B, Gmax, K): proposal rows, -1 pad.
__global__ __launch_bounds__(256) void near_targets_kernel(const float* __restrict__ proposals,
                                                           const int* __restrict__ bag_off,
                                                           const int* __restrict__ labels, int bg_label,
                                                           const float* __restrict__ pgt_box,
                                                           const int* __restrict__ counts, int Gmax, int K,
                                                           int* __restrict__ near_rows) {
  __shared__ BestPair slot[4];
  const int img = blockIdx.x / Gmax, g = blockIdx.x % Gmax;
  int* out = near_rows + (size_t)blockIdx.x * K;
  if (g >= counts[img]) {
    for (int k = threadIdx.x; k < K; k += blockDim.x) out[k] = -1;
    return;
  }
  const int r0 = bag_off[img], r1 = bag_off[img + 1];
  const float4 q = box_at(pgt_box, (long)img * Gmax + g);
  float li = 2.f;                                                       // the previous pick (uniform)
  int lr = -1;
  for (int k = 0; k < K; ++k) {
    float best = -1.f;
    int at = kNoIndex;
    for (int r = r0 + threadIdx.x; r < r1; r += blockDim.x) {
      if (labels[r] == bg_label || labels[r] < 0) continue;           // foreground proposals only
      const float v = box_iou(q, box_at(proposals, r));               // (target, proposal)
      const bool after = v < li || (v == li && r > lr);               // strictly after the previous pick
      if (after && (v > best || (v == best && r < at))) { best = v; at = r; }
    }
    const BestPair top = wg_arg_best<4>(best, at, slot);
    const bool found = best_index(top) != kNoIndex;
    if (threadIdx.x == 0) out[k] = found ? best_index(top) : -1;
    li = found ? best_value(top) : -2.f;                               // exhausted: nothing comes after
    lr = best_index(top);
  }
}

// Second labelling pass against the near targets (label_and_sample_proposals(instances, near_targets),
// roi_heads_jtsm.py:893-905 -> roi_heads.py:306-340): each foreground proposal takes the mask of the near target with
// the highest IoU (first maximum in list order: pseudo box major, rank minor).  matched_near[r] = that target's
// proposal row (-1 for non-foreground proposals / images without targets).
__global__ __launch_bounds__(256) void match_near_kernel(const float* __restrict__ proposals, const int* __restrict__ bag_off,
                                                         int B, int R, const int* __restrict__ labels, int bg_label,
                                                         const int* __restrict__ near_rows, const int* __restrict__ counts,
                                                         int Gmax, int K, int* __restrict__ matched_near) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  if (labels[r] == bg_label || labels[r] < 0) { matched_near[r] = -1; return; }
  const int img = image_of(bag_off, B, r);
  const float4 p = box_at(proposals, r);
  float best = -1.f;
  int at = -1;
  const int n = counts[img];
  for (int g = 0; g < n; ++g)
    for (int k = 0; k < K; ++k) {
      const int row = near_rows[((size_t)img * Gmax + g) * K + k];
      if (row < 0) break;
      const float v = box_iou(box_at(proposals, row), p);                 // (target, proposal)
      if (v > best) { best = v; at = row; }
    }
  matched_near[r] = at;
}

// ---- pseudo semantic target (get_pgt_sem_seg, roi_heads_jtsm.py:2025-2070): every pseudo target paints the pixels it
// covers with value class - class_base, in ascending score order (the best target ends on top); then, in list order, a
// class whose pixels were all painted over is painted once more.  The top pass is pixel-parallel (max score RANK among
// the covering targets) and counts the pixels of every value; the missing pass (one workgroup per image) replays the
// sequential "missing class" rule on those counts, touching only the pixels it repaints.  No host synchronisation:
// list lengths stay on the device.  What a target covers is the Cover policy's:
//   RectCover      the rectangle substitution of SURVEY F8: the target's box shrunk by `erode` pixels; a repaint walks
//                  the eroded box's bounding rectangle.
//   EvidenceCover  the reference's masks (need_mask=True -> get_pgt_top_k :1333-1334 -> object_evidence :1928-1994,
//                  superpixel branch): the union of the superpixels the target's oh_labels row marks,
//                  mask_j(y, x) = oh_labels[row_j][superpixels[y][x]] != 0 (a superpixel id outside [0, L) belongs to no
//                  mask: the reference's `poses` loop covers range(L) only); a repaint walks the whole image.  The
//                  full-image masks are never rasterised.
// A policy names its per-target state (Target, staged in LDS by the top pass), what it reads of a pixel (Pixel, with
// its flat index `at`), the pixels a repaint of one target walks (Domain) and the coverage test.
constexpr int kPaintValues = 64;   // painted values are 1 .. 63 (0 = untouched)
constexpr int kPaintTargets = 64;  // targets per image

struct RectCover {
  const float* __restrict__ boxes;   // (B, G, 4)
  float erode;
  struct Target { float b[4]; };
  struct Pixel { long at; int x, y; };
  struct Domain { int x0, y0, bw; long count; };
  __device__ Target target(int b, int G, int j) const {
    Target t;
    for (int e = 0; e < 4; ++e) t.b[e] = boxes[((size_t)b * G + j) * 4 + e];
    return t;
  }
  __device__ Pixel pixel(int, long at, int, int W) const {
    const int y = (int)(at / W);
    return {at, (int)(at - (long)y * W), y};
  }
  __device__ Domain domain(const Target& t, int H, int W) const {
    const int x0 = max(0, (int)floorf(t.b[0] + erode - 0.5f)), x1 = min(W - 1, (int)ceilf(t.b[2] - erode - 0.5f));
    const int y0 = max(0, (int)floorf(t.b[1] + erode - 0.5f)), y1 = min(H - 1, (int)ceilf(t.b[3] - erode - 0.5f));
    const int bw = x1 - x0 + 1, bh = y1 - y0 + 1;
    return {x0, y0, bw, bw > 0 && bh > 0 ? (long)bw * bh : 0};
  }
  __device__ Pixel pixel_of(int, const Domain& d, long i, int, int W) const {
    const int y = d.y0 + (int)(i / d.bw), x = d.x0 + (int)(i % d.bw);
    return {(long)y * W + x, x, y};
  }
  __device__ bool covers(const Target& t, const Pixel& p) const {
    const float xs = (float)p.x + 0.5f, ys = (float)p.y + 0.5f;
    return xs >= t.b[0] + erode && xs <= t.b[2] - erode && ys >= t.b[1] + erode && ys <= t.b[3] - erode;
  }
};

struct EvidenceCover {
  const int* __restrict__ target_idx;    // (B, G) row of the target within its image
  const int* __restrict__ bag_offsets;
  const int* __restrict__ oh_labels;     // (R, L)
  int L;
  const int* __restrict__ superpixels;   // (B, H, W)
  struct Target { const int* row; };
  struct Pixel { long at; int s; };      // s: the pixel's superpixel, -1 when it is outside [0, L)
  struct Domain { long count; };
  __device__ Target target(int b, int G, int j) const {
    return {oh_labels + ((long)bag_offsets[b] + target_idx[b * G + j]) * L};
  }
  __device__ Pixel pixel(int b, long at, int H, int W) const {
    const int s = superpixels[(size_t)b * H * W + at];
    return {at, s >= 0 && s < L ? s : -1};
  }
  __device__ Domain domain(const Target&, int H, int W) const { return {(long)H * W}; }
  __device__ Pixel pixel_of(int b, const Domain&, long i, int H, int W) const { return pixel(b, i, H, W); }
  __device__ bool covers(const Target& t, const Pixel& p) const { return p.s >= 0 && t.row[p.s] != 0; }
};

template <class Cover>
__global__ __launch_bounds__(256) void paint_top_kernel(const Cover cover, const int* __restrict__ classes,
                                                        const float* __restrict__ scores, const int* __restrict__ counts,
                                                        int G, int class_base, int H, int W, long* __restrict__ out,
                                                        int* __restrict__ value_counts) {
  __shared__ int hist[kPaintValues];
  __shared__ typename Cover::Target starget[kPaintTargets];
  __shared__ int srank[kPaintTargets], sval[kPaintTargets];
  const int b = blockIdx.y, n = min(counts[b], kPaintTargets);
  if (threadIdx.x < kPaintValues) hist[threadIdx.x] = 0;
  if (threadIdx.x < n) {
    const int j = threadIdx.x;
    const float sj = scores[b * G + j];
    int r = 0;   // position of target j in ascending (score, index) order
    for (int k = 0; k < n; ++k) {
      const float sk = scores[b * G + k];
      r += (sk < sj || (sk == sj && k < j)) ? 1 : 0;
    }
    srank[j] = r;
    sval[j] = classes[b * G + j] - class_base;
    starget[j] = cover.target(b, G, j);
  }
  __syncthreads();
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p < (long)H * W) {
    const typename Cover::Pixel px = cover.pixel(b, p, H, W);
    int best = -1, val = 0;
    for (int j = 0; j < n; ++j)   // the highest rank that covers the pixel
      if (srank[j] > best && cover.covers(starget[j], px)) { best = srank[j]; val = sval[j]; }
    out[(size_t)b * H * W + p] = val;
    atomicAdd(&hist[val & (kPaintValues - 1)], 1);
  }
  __syncthreads();
  if (threadIdx.x < kPaintValues && hist[threadIdx.x]) atomicAdd(value_counts + b * kPaintValues + threadIdx.x, hist[threadIdx.x]);
}

template <class Cover, int THREADS>
__global__ __launch_bounds__(THREADS) void paint_missing_kernel(const Cover cover, const int* __restrict__ classes,
                                                                const int* __restrict__ counts, int G, int class_base,
                                                                int H, int W, long* __restrict__ out,
                                                                const int* __restrict__ value_counts) {
  __shared__ int cnt[kPaintValues];
  const int b = blockIdx.x, n = min(counts[b], kPaintTargets);
  if (threadIdx.x < kPaintValues) cnt[threadIdx.x] = value_counts[b * kPaintValues + threadIdx.x];
  __syncthreads();
  long* img = out + (size_t)b * H * W;
  for (int j = 0; j < n; ++j) {
    const int v = (classes[b * G + j] - class_base) & (kPaintValues - 1);
    const bool missing = cnt[v] == 0;   // uniform: read before anyone updates it in this round
    __syncthreads();
    if (missing) {
      const typename Cover::Target t = cover.target(b, G, j);
      const typename Cover::Domain d = cover.domain(t, H, W);
      for (long i = threadIdx.x; i < d.count; i += THREADS) {
        const typename Cover::Pixel px = cover.pixel_of(b, d, i, H, W);
        if (!cover.covers(t, px)) continue;
        const long old = img[px.at];
        img[px.at] = v;
        atomicSub(&cnt[(int)old & (kPaintValues - 1)], 1);
        atomicAdd(&cnt[v], 1);
      }
    }
    __syncthreads();
  }
}

// The two passes of one painter; value_counts (B, kPaintValues) is the workspace.
template <class Cover, int MISSING_THREADS>
int paint_sem_seg(const Cover& cover, const int* classes, const float* scores, const int* counts, int B, int G,
                  int class_base, int H, int W, int64_t* out, void* workspace, void* stream, const char* what) {
  hipStream_t st = as_stream(stream);
  int* value_counts = reinterpret_cast<int*>(workspace);
  JTSM_CHECK_HIP(hipMemsetAsync(value_counts, 0, (size_t)B * kPaintValues * sizeof(int), st));
  const long hw = (long)H * W;
  hipLaunchKernelGGL((paint_top_kernel<Cover>), dim3((unsigned)((hw + 255) / 256), B), dim3(256), 0, st, cover, classes,
                     scores, counts, G, class_base, H, W, reinterpret_cast<long*>(out), value_counts);
  hipLaunchKernelGGL((paint_missing_kernel<Cover, MISSING_THREADS>), dim3(B), dim3(MISSING_THREADS), 0, st, cover, classes,
                     counts, G, class_base, H, W, reinterpret_cast<long*>(out), value_counts);
  JTSM_CHECK_LAUNCH(what);
  return JTSM_OK;
}


// ---------------------------------------------------------------------------------------------------------------
// Label preparation in three launches (round 3).  What these replace were ~80 PyTorch device launches of a few hundred
// threads each per step (arange / where / sort / remainder / index_put / sqrt / log2 / floor / clamp / cat ...), 2-5 us
// apiece on a busy device.  Per-image inputs arrive as up to kMaxImages pointers BY VALUE in the kernel arguments: no
// concatenation and no table upload.
constexpr int kMaxImages = 16;
struct ImageRows {
  const void* ptr[kMaxImages];
  int first[kMaxImages + 1];      // first[b] .. first[b + 1]: the rows of image b in the concatenation
};

// detectron2 poolers.py:22-58 + 61-95 as ONE pass: rois (M,5) = [image, x0, y0, x1, y1] and the 0-based level
//   floor(canonical_level + log2(sqrt(area) / canonical_size + 1e-8)) clamped to [min_level, max_level] (NaN -> min).
// The arithmetic is PyTorch's, operation by operation (its division by a host scalar is a multiplication by the
// rounded reciprocal), so the levels are the ones `assign_boxes_to_levels` computes.
__global__ __launch_bounds__(256) void pooler_rois_levels_kernel(const ImageRows im, int B, int M, float inv_canonical,
                                                                 float canonical_level, int min_level, int max_level,
                                                                 float* __restrict__ rois, int* __restrict__ level) {
#pragma clang fp contract(off)
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const int b = image_of(im.first, B, m);
  const float4 bx = reinterpret_cast<const float4*>(im.ptr[b])[m - im.first[b]];
  rois[(size_t)m * 5 + 0] = (float)b;
  rois[(size_t)m * 5 + 1] = bx.x; rois[(size_t)m * 5 + 2] = bx.y;
  rois[(size_t)m * 5 + 3] = bx.z; rois[(size_t)m * 5 + 4] = bx.w;
  const float area = (bx.z - bx.x) * (bx.w - bx.y);
  float lv = floorf(canonical_level + log2f(sqrtf(area) * inv_canonical + 1e-8f));
  if (lv != lv) lv = (float)min_level;
  lv = fminf(fmaxf(lv, (float)min_level), (float)max_level);
  level[m] = (int)lv - min_level;
}

// roi_heads_jtsm.py:607-633 glue: scale[m] = bins / (nvalid[m] + 1) * (objectness[m] + 1), nvalid = the bins of roi m
// whose MOIPool arg-max (channel 0) is not -1.  arg: (M, bins, C) int32 (channels-last).  Operation order as in the
// PyTorch expression it replaces: (bins * (1 / (nvalid + 1))) * (objectness + 1).
__global__ __launch_bounds__(256) void roi_scale_kernel(const int* __restrict__ arg, int bins, int C, const ImageRows obj,
                                                        int B, int M, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  int nvalid = 0;
  for (int i = 0; i < bins; ++i) nvalid += arg[((size_t)m * bins + i) * C] != -1;
  const int b = image_of(obj.first, B, m);
  const float o = reinterpret_cast<const float*>(obj.ptr[b])[m - obj.first[b]];
  out[m] = ((float)bins * (1.0f / ((float)nvalid + 1.0f))) * (o + 1.0f);
}

// which of the labels 0..255 occur in each image's semantic map (values outside are clamped, as the scatter it
// replaces clamps them).  flags (B,256) int32, zeroed by the caller.
template <typename T>
__global__ __launch_bounds__(256) void sem_label_flags_kernel(const T* __restrict__ sem, long pixels, int* __restrict__ flags) {
  __shared__ int seen[256];
  seen[threadIdx.x] = 0;
  __syncthreads();
  const T* img = sem + (size_t)blockIdx.y * pixels;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += (long)gridDim.x * blockDim.x) {
    long v = (long)img[i];
    v = v < 0 ? 0 : (v > 255 ? 255 : v);
    seen[v] = 1;            // (racing stores of the same value)
  }
  __syncthreads();
  if (seen[threadIdx.x]) flags[blockIdx.y * 256 + threadIdx.x] = 1;
}

// one-hot row, class list (present classes ascending, then the absent ones ascending, each + offset: what
// sort(where(present, c, c + C)) % C + offset gives) and count of one image.  C <= 256.
__device__ __forceinline__ void emit_class_list(bool present, int c, int C, int offset, float* __restrict__ oh,
                                                int* __restrict__ cls, int* __restrict__ cnt, int* wave_count) {
  int npresent, nabsent;
  const bool valid = c < C;
  const int ps = compact_wg<4>(valid && present, wave_count, npresent);
  const int as = compact_wg<4>(valid && !present, wave_count, nabsent);
  if (valid) {
    oh[c] = present ? 1.f : 0.f;
    cls[present ? ps : npresent + as] = c + offset;
  }
  if (c == 0) *cnt = npresent;
}
__global__ __launch_bounds__(256) void image_class_lists_kernel(const ImageRows things, int C, const int* __restrict__ stuff_flags,
                                                                int S, int stuff_offset, float* __restrict__ oh_things,
                                                                int* __restrict__ things_cls, int* __restrict__ things_cnt,
                                                                float* __restrict__ oh_stuff, int* __restrict__ stuff_cls,
                                                                int* __restrict__ stuff_cnt) {
  __shared__ int seen[256];
  __shared__ int wave_count[4];
  const int b = blockIdx.x, t = threadIdx.x;
  seen[t] = 0;
  __syncthreads();
  const long* gt = reinterpret_cast<const long*>(things.ptr[b]);
  const int n = things.first[b + 1] - things.first[b];
  for (int i = t; i < n; i += 256) {
    const long c = gt[i];
    if (c >= 0 && c < C) seen[c] = 1;
  }
  __syncthreads();
  emit_class_list(seen[t] != 0, t, C, 0, oh_things + (size_t)b * C, things_cls + (size_t)b * C, things_cnt + b, wave_count);
  if (stuff_flags)   // stuff label l = 1 .. S - 1 is column l - 1 (0 = things and 255 = ignore do not count)
    emit_class_list(t + 1 < 256 && stuff_flags[b * 256 + t + 1] != 0, t, S - 1, stuff_offset, oh_stuff + (size_t)b * (S - 1),
                    stuff_cls + (size_t)b * (S - 1), stuff_cnt + b, wave_count);
}


// The mask branch trains on the foreground proposals only (roi_heads_jtsm.py:754-948): their rows, in row order, with
// what the branch reads of them — one workgroup, an ordered compaction 1024 rows at a time.  fg_* hold `total` valid
// entries (a host-side slice after the count has crossed: no kernel), counts[b] = foreground rows of image b.
__global__ __launch_bounds__(1024) void fg_compact_kernel(const int* __restrict__ labels, int bg_label, const int* __restrict__ bag_offsets,
                                                          int B, int R, const float* __restrict__ boxes,
                                                          const int* __restrict__ matched, int* __restrict__ fg_rows,
                                                          float* __restrict__ fg_boxes, long* __restrict__ fg_classes,
                                                          int* __restrict__ fg_img, int* __restrict__ fg_matched,
                                                          float* __restrict__ fg_rois, long* __restrict__ counts) {
  __shared__ int wave_count[16];
  __shared__ int per_image[64];
  const int t = threadIdx.x;
  if (t < 64) per_image[t] = 0;
  __syncthreads();
  int filled = 0;
  for (int base = 0; base < R; base += 1024) {
    const int r = base + t;
    const int lab = r < R ? labels[r] : bg_label;
    const bool fg = lab != bg_label;
    int cnt;
    const int slot = filled + compact_wg<16>(fg, wave_count, cnt);
    if (fg) {
      const int b = image_of(bag_offsets, B, r);
      const float4 bx = load_box(boxes, r);
      fg_rows[slot] = r;
      reinterpret_cast<float4*>(fg_boxes)[slot] = bx;
      fg_classes[slot] = lab;
      fg_img[slot] = b;
      if (matched) fg_matched[slot] = matched[r];
      fg_rois[(size_t)slot * 5 + 0] = (float)b;
      fg_rois[(size_t)slot * 5 + 1] = bx.x; fg_rois[(size_t)slot * 5 + 2] = bx.y;
      fg_rois[(size_t)slot * 5 + 3] = bx.z; fg_rois[(size_t)slot * 5 + 4] = bx.w;
      atomicAdd(&per_image[b], 1);
    }
    filled += cnt;
  }
  __syncthreads();
  if (t < B) counts[t] = per_image[t];
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" {

int jtsm_row_lse_f32(const float* logits, int ld, int ncls, int R, float* lse, void* stream) {
  JTSM_REQUIRE(R >= 0 && ncls > 0 && ld >= ncls, "row_lse: bad sizes");
  if (R == 0) return JTSM_OK;
  JTSM_REQUIRE(logits && lse, "row_lse: null pointer");
  hipLaunchKernelGGL(row_lse_kernel, dim3(ceil_div(R, 4)), dim3(256), 0, as_stream(stream), logits, ld, ncls, R, lse);
  JTSM_CHECK_LAUNCH("row_lse");
  return JTSM_OK;
}

int jtsm_mine_top1_f32(const float* scores, int ld, const float* lse, const float* proposals, const float* deltas,
                       int ld_deltas, const int32_t* bag_offsets, const int32_t* classes, const int32_t* counts,
                       int B, int Gmax, const float* img_probs, int nprob, int32_t* out_idx, float* out_box,
                       float* out_score, float* out_weight, void* stream) {
  JTSM_REQUIRE(B >= 0 && Gmax >= 0, "mine_top1: bad sizes");
  if (B == 0 || Gmax == 0) return JTSM_OK;
  JTSM_REQUIRE(scores && proposals && bag_offsets && classes && counts && img_probs && out_idx && out_box &&
               out_score && out_weight, "mine_top1: null pointer");
  hipLaunchKernelGGL(mine_top1_kernel, dim3(B * Gmax), dim3(256), 0, as_stream(stream), scores, ld, lse, proposals,
                     deltas, ld_deltas, bag_offsets, classes, counts, Gmax, img_probs, nprob, out_idx, out_box,
                     out_score, out_weight);
  JTSM_CHECK_LAUNCH("mine_top1");
  return JTSM_OK;
}

int jtsm_match_label_f32(const float* proposals, const int32_t* bag_offsets, int B, int R, const float* pgt_box,
                         const int32_t* classes, const int32_t* counts, const float* pgt_weight,
                         const float* pgt_score, int Gmax, float iou_thresh, int bg_label, int32_t* labels,
                         int32_t* matched, float* gt_boxes, float* gt_weights, float* gt_scores, void* stream) {
  JTSM_REQUIRE(B > 0 && R >= 0 && Gmax >= 0, "match_label: bad sizes");
  if (R == 0) return JTSM_OK;
  JTSM_REQUIRE(proposals && bag_offsets && pgt_box && classes && counts && pgt_weight && labels && matched &&
               gt_boxes && gt_weights, "match_label: null pointer");
  hipLaunchKernelGGL(match_label_kernel, dim3(ceil_div(R, 256)), dim3(256), 0, as_stream(stream), proposals,
                     bag_offsets, B, R, pgt_box, classes, counts, pgt_weight, pgt_score, Gmax, iou_thresh, bg_label,
                     labels, matched, gt_boxes, gt_weights, gt_scores);
  JTSM_CHECK_LAUNCH("match_label");
  return JTSM_OK;
}

int jtsm_near_targets_f32(const float* proposals, const int32_t* bag_offsets, int B, int R, const int32_t* labels,
                          int bg_label, const float* pgt_box, const int32_t* counts, int Gmax, int top_k,
                          int32_t* near_rows, int32_t* matched_near, void* stream) {
  JTSM_REQUIRE(B > 0 && R >= 0 && Gmax > 0 && top_k > 0 && top_k <= 64, "near_targets: bad sizes");
  JTSM_REQUIRE(proposals && bag_offsets && labels && pgt_box && counts && near_rows && matched_near,
               "near_targets: null pointer");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(near_targets_kernel, dim3(B * Gmax), dim3(256), 0, st, proposals, bag_offsets, labels, bg_label,
                     pgt_box, counts, Gmax, top_k, near_rows);
  if (R > 0)
    hipLaunchKernelGGL(match_near_kernel, dim3(ceil_div(R, 256)), dim3(256), 0, st, proposals, bag_offsets, B, R, labels,
                       bg_label, near_rows, counts, Gmax, top_k, matched_near);
  JTSM_CHECK_LAUNCH("near_targets");
  return JTSM_OK;
}

size_t jtsm_paint_sem_seg_workspace_bytes(int B) { return (size_t)(B > 0 ? B : 0) * kPaintValues * sizeof(int) + 16; }

int jtsm_paint_sem_seg(const float* boxes, const int32_t* classes, const float* scores, const int32_t* counts, int B,
                       int G, int class_base, int H, int W, float erode, int64_t* out, void* workspace, void* stream) {
  JTSM_REQUIRE(B >= 0 && G > 0 && G <= 64 && H > 0 && W > 0, "paint_sem_seg: bad sizes (at most 64 boxes per image)");
  if (B == 0) return JTSM_OK;
  JTSM_REQUIRE(boxes && classes && scores && counts && out && workspace, "paint_sem_seg: null pointer");
  return paint_sem_seg<RectCover, 256>({boxes, erode}, classes, scores, counts, B, G, class_base, H, W, out, workspace,
                                       stream, "paint_sem_seg");
}

int jtsm_paint_sem_seg_evidence(const int32_t* target_idx, const int32_t* bag_offsets, const int32_t* oh_labels, int L,
                                const int32_t* superpixels, const int32_t* classes, const float* scores,
                                const int32_t* counts, int B, int G, int class_base, int H, int W, int64_t* out,
                                void* workspace, void* stream) {
  JTSM_REQUIRE(B >= 0 && G > 0 && G <= 64 && H > 0 && W > 0 && L > 0,
               "paint_sem_seg_evidence: bad sizes (at most 64 targets per image)");
  if (B == 0) return JTSM_OK;
  JTSM_REQUIRE(target_idx && bag_offsets && oh_labels && superpixels && classes && scores && counts && out && workspace,
               "paint_sem_seg_evidence: null pointer");
  return paint_sem_seg<EvidenceCover, 1024>({target_idx, bag_offsets, oh_labels, L, superpixels}, classes, scores, counts,
                                            B, G, class_base, H, W, out, workspace, stream, "paint_sem_seg_evidence");
}

namespace {
int pack_rows(const void* const* ptrs, const int* counts, int B, jtsm::ImageRows& out, int& total) {
  JTSM_REQUIRE(B >= 1 && B <= jtsm::kMaxImages, "label preparation: 1..%d images per call, got %d", jtsm::kMaxImages, B);
  total = 0;
  for (int b = 0; b < jtsm::kMaxImages; ++b) { out.ptr[b] = nullptr; out.first[b] = 0; }
  for (int b = 0; b < B; ++b) {
    JTSM_REQUIRE(counts[b] >= 0 && (counts[b] == 0 || ptrs[b]), "label preparation: image %d has %d rows at %p", b, counts[b], ptrs[b]);
    out.ptr[b] = ptrs[b];
    out.first[b] = total;
    total += counts[b];
  }
  for (int b = B; b <= jtsm::kMaxImages; ++b) out.first[b] = total;
  return JTSM_OK;
}
}  // namespace

int jtsm_pooler_rois_levels_f32(const float* const* boxes, const int* counts, int B, int min_level, int max_level,
                                float canonical_box_size, float canonical_level, float* rois, int32_t* level, void* stream) {
  jtsm::ImageRows im;
  int M;
  if (int rc = pack_rows(reinterpret_cast<const void* const*>(boxes), counts, B, im, M)) return rc;
  JTSM_REQUIRE(canonical_box_size > 0.f && min_level <= max_level, "pooler levels: bad canonical size / level range");
  for (int b = 0; b < B; ++b)
    JTSM_REQUIRE((reinterpret_cast<uintptr_t>(boxes[b]) & 15) == 0, "pooler levels: image %d's boxes are not 16-byte aligned", b);
  if (M == 0) return JTSM_OK;
  hipLaunchKernelGGL(jtsm::pooler_rois_levels_kernel, dim3(jtsm::ceil_div(M, 256)), dim3(256), 0, jtsm::as_stream(stream), im, B, M,
                     1.0f / canonical_box_size, canonical_level, min_level, max_level, rois, level);
  JTSM_CHECK_LAUNCH("pooler_rois_levels");
  return JTSM_OK;
}

int jtsm_roi_scale_f32(const int32_t* argmax, int bins, int C, const float* const* objectness, const int* counts, int B,
                       float* out, void* stream) {
  jtsm::ImageRows im;
  int M;
  if (int rc = pack_rows(reinterpret_cast<const void* const*>(objectness), counts, B, im, M)) return rc;
  JTSM_REQUIRE(bins > 0 && C > 0, "roi_scale: bins %d, channels %d", bins, C);
  if (M == 0) return JTSM_OK;
  hipLaunchKernelGGL(jtsm::roi_scale_kernel, dim3(jtsm::ceil_div(M, 256)), dim3(256), 0, jtsm::as_stream(stream), argmax, bins, C, im,
                     B, M, out);
  JTSM_CHECK_LAUNCH("roi_scale");
  return JTSM_OK;
}

size_t jtsm_image_labels_workspace_bytes(int B) { return (size_t)(B > 0 ? B : 0) * 256 * sizeof(int); }

int jtsm_image_labels(const int64_t* const* gt_classes, const int* counts, int B, int num_classes, const void* sem_seg,
                      int sem_elem_bytes, long pixels, int num_stuff, int stuff_offset, float* oh_things,
                      int32_t* things_cls, int32_t* things_cnt, float* oh_stuff, int32_t* stuff_cls, int32_t* stuff_cnt,
                      void* workspace, void* stream) {
  jtsm::ImageRows im;
  int total;
  if (int rc = pack_rows(reinterpret_cast<const void* const*>(gt_classes), counts, B, im, total)) return rc;
  JTSM_REQUIRE(num_classes >= 1 && num_classes <= 256, "image labels: 1..256 thing classes, got %d", num_classes);
  int* flags = nullptr;
  if (sem_seg) {
    JTSM_REQUIRE(num_stuff >= 2 && num_stuff <= 256 && pixels > 0 && workspace && (sem_elem_bytes == 8 || sem_elem_bytes == 1),
                 "image labels: stuff classes %d, %ld pixels, %d-byte labels", num_stuff, pixels, sem_elem_bytes);
    flags = reinterpret_cast<int*>(workspace);
    JTSM_CHECK_HIP(hipMemsetAsync(flags, 0, jtsm_image_labels_workspace_bytes(B), jtsm::as_stream(stream)));
    const dim3 grid((unsigned)(pixels / 256 / 16 < 1 ? 1 : (pixels / 256 / 16 > 256 ? 256 : pixels / 256 / 16)), B);
    if (sem_elem_bytes == 8)
      hipLaunchKernelGGL((jtsm::sem_label_flags_kernel<long>), grid, dim3(256), 0, jtsm::as_stream(stream),
                         reinterpret_cast<const long*>(sem_seg), pixels, flags);
    else
      hipLaunchKernelGGL((jtsm::sem_label_flags_kernel<unsigned char>), grid, dim3(256), 0, jtsm::as_stream(stream),
                         reinterpret_cast<const unsigned char*>(sem_seg), pixels, flags);
    JTSM_CHECK_LAUNCH("sem_label_flags");
  }
  hipLaunchKernelGGL(jtsm::image_class_lists_kernel, dim3(B), dim3(256), 0, jtsm::as_stream(stream), im, num_classes, flags, num_stuff,
                     stuff_offset, oh_things, things_cls, things_cnt, oh_stuff, stuff_cls, stuff_cnt);
  JTSM_CHECK_LAUNCH("image_class_lists");
  return JTSM_OK;
}

int jtsm_fg_compact(const int32_t* labels, int bg_label, const int32_t* bag_offsets, int B, int R, const float* boxes,
                    const int32_t* matched, int32_t* fg_rows, float* fg_boxes, int64_t* fg_classes, int32_t* fg_img,
                    int32_t* fg_matched, float* fg_rois, int64_t* counts, void* stream) {
  JTSM_REQUIRE(B >= 1 && B <= 64 && R >= 0, "fg_compact: 1..64 images, got %d (rows %d)", B, R);
  JTSM_REQUIRE(labels && bag_offsets && boxes && fg_rows && fg_boxes && fg_classes && fg_img && fg_rois && counts &&
               (!matched || fg_matched), "fg_compact: null pointer");
  JTSM_REQUIRE((reinterpret_cast<uintptr_t>(boxes) & 15) == 0 && (reinterpret_cast<uintptr_t>(fg_boxes) & 15) == 0,
               "fg_compact: boxes must be 16-byte aligned");
  hipLaunchKernelGGL(jtsm::fg_compact_kernel, dim3(1), dim3(1024), 0, jtsm::as_stream(stream), labels, bg_label, bag_offsets, B, R,
                     boxes, matched, fg_rows, fg_boxes, reinterpret_cast<long*>(fg_classes), fg_img, fg_matched, fg_rois,
                     reinterpret_cast<long*>(counts));
  JTSM_CHECK_LAUNCH("fg_compact");
  return JTSM_OK;
}

}  // extern "C"
