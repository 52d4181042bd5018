// PCL (proposal cluster learning) for gfx950: proposal clustering and the PCL loss, all on the device.
//
// Replaces, per refinement branch,
//   PCL(boxes, cls_prob, im_labels, cls_prob_new)  projects/WSL/wsl/modeling/roi_heads/third_party/pcl.py:24-200
//     (host numpy + scikit-learn KMeans, after a device -> host copy of the probabilities), and
//   pcl_loss_forward / pcl_loss_backward            projects/WSL/wsl/layers/csrc/pcl_loss/pcl_loss_cpu.cpp:8-115
//     (the CPU kernel is the one that runs: wsl/layers/pcl_loss.py:23-51 calls .cpu() first).
//
// Per image (rows [offsets[i], offsets[i+1]) of every per-proposal array; K classes, background in column 0 of the
// branch's own probabilities):
//   prev  = the previous branch's probabilities of the K classes, clipped to [1e-9f, (float)(1 - 1e-9)] (pcl.py:29-35)
//   probs = this branch's soft-max probabilities (R, K+1), clipped the same way where pc_prob reads them
//   for each present class c, ascending (pcl.py:95-139):
//     top-ranking set: a deterministic 1-D Lloyd iteration on prev[:, c] over the candidate pool — the DECLARED
//       substitution for KMeans(n_clusters=min(3,n), random_state=3): centres start at min, midpoint, max
//       (n = 2: min, max; n = 1: the one proposal is the set); a value goes to the nearest centre, ties to the lower
//       centre; means in fp64; an empty cluster keeps its centre; stop when no assignment changes or after 300 passes;
//       the set is the cluster of the largest centre (the first of equal centres); empty -> the arg-max proposal
//     graph: edge where IoU > 0.4f (pairwise_iou, no +1), every box has an edge to itself
//     do { node of largest degree among the remaining nodes — LOWEST INDEX among equal degrees (the reference's
//          unstable argsort leaves this open); its score = the largest prev probability over it and its
//          remaining neighbours; remove them } while (more than 5 nodes remain)
//     keep the 5 best-scoring centres in descending order of score — the EARLIER-PICKED centre among equal scores;
//     the kept centres' proposals leave the pool of the later classes
//   clusters (pcl.py:146-200): every proposal goes to its highest-IoU centre (first maximum); IoU < 0.5f: label 0,
//     assignment -1; IoU < 0.1f: weight 0; else weight = the centre's score.  Per cluster: label, member count, summed
//     member weight, pc_prob = mean of the members' clipped probability of the cluster's class (fp64 sum in a fixed
//     order, rounded once).  A cluster without members has count 0 and contributes nothing.
// Loss (pcl_loss_cpu.cpp): per image  ( -sum_{label=0} w log max(p0, 1e-6) - sum_j W_j log max(pc_prob_j, 1e-6) ) / R_i,
//   mean over the images.  Gradient to the probabilities: background rows -w / max(p0, 1e-5) in column 0, members
//   -W_j / max(count_j pc_prob_j, 1e-5) in column label; divided by R_i and by the number of images, multiplied by the
//   upstream gradient, and carried through the soft-max to the logits in the same kernel.
//
// No float atomics anywhere: every sum is a strided per-thread sum followed by a butterfly and a fixed-order fold, so
// the same inputs give the same tables on every run.
#include <algorithm>

#include "mining_common.h"
#include "reduce.h"
#include "workspace.h"

namespace jtsm {
namespace {

#pragma clang fp contract(off)

constexpr int kThreads = 1024;          // one workgroup per image in the centre search
constexpr int kRowsPerThread = 8;       // rows of an image a thread of that workgroup owns
constexpr int kMaxRows = kThreads * kRowsPerThread;
constexpr int kMaxPC = 5;               // cfg_TRAIN_MAX_PC_NUM
constexpr int kLloydPasses = 300;       // scikit-learn's max_iter
constexpr float kGraphIou = 0.4f, kFgIou = 0.5f, kBgIou = 0.1f;
constexpr float kClipLo = 1e-9f, kClipHi = (float)(1.0 - 1e-9);

using u64 = unsigned long long;

__device__ __forceinline__ float clip_prob(float v) { return fminf(fmaxf(v, kClipLo), kClipHi); }

// (box_iou — detectron2's pairwise_iou, un-contracted — and load_box: box_math.h)

// (wg_reduce and its ops: reduce.h; index_key / key_index — an arg-max whose LOWEST index wins ties: common.h)

// ---- centre search: one workgroup of 1024 per image ------------------------------------------------------------------
// ws_adj: (max_rows, words) u64 adjacency rows of the top-ranking set; ws_keep_node / ws_keep_score: the centres the
// greedy search picked, in order.
__global__ __launch_bounds__(kThreads) void pcl_centres_kernel(
    const float* __restrict__ boxes, const int* __restrict__ offsets, const float* __restrict__ prev, int ld_prev,
    int prev_col0, const float* __restrict__ labels, int K, int maxc, int max_rows, u64* __restrict__ ws_adj,
    int* __restrict__ ws_keep_node, float* __restrict__ ws_keep_score, int* __restrict__ pc_int,
    float* __restrict__ pc_flt, int* __restrict__ pc_num) {
#pragma clang fp contract(off)
  __shared__ unsigned char pool[kMaxRows];          // 1: still in the candidate pool
  __shared__ unsigned short tlist[kMaxRows];        // the top-ranking set, ascending rows
  __shared__ u64 alive[kMaxRows / 64];
  __shared__ u64 slot_u[kThreads / 64];
  __shared__ double slot_d[kThreads / 64];
  __shared__ float slot_f[kThreads / 64];
  __shared__ int wave_count[kThreads / 64];

  const int img = blockIdx.x, t = threadIdx.x;
  const int off = offsets[img], R = offsets[img + 1] - off;
  const int words_max = (max_rows + 63) / 64;
  u64* __restrict__ adj = ws_adj + (size_t)img * max_rows * words_max;
  int* __restrict__ keep_node = ws_keep_node + (size_t)img * max_rows;
  float* __restrict__ keep_score = ws_keep_score + (size_t)img * max_rows;
  int* __restrict__ pci = pc_int + (size_t)img * maxc * 3;
  float* __restrict__ pcf = pc_flt + (size_t)img * maxc * 3;
  for (int j = t; j < maxc * 3; j += kThreads) { pci[j] = 0; pcf[j] = 0.f; }
  for (int r = t; r < kMaxRows; r += kThreads) pool[r] = r < R;
  int G = 0;                                         // centres so far (uniform)
  __syncthreads();
  if (R > max_rows || R > kMaxRows) {                // (the host checks the bound it is given; never index past it)
    if (t == 0) pc_num[img] = 0;
    return;
  }

  for (int c = 0; c < K && R > 0; ++c) {
    if (labels[(size_t)img * K + c] != 1.f) continue;                       // (uniform)
    const float* __restrict__ col = prev + (size_t)off * ld_prev + prev_col0 + c;
    // ---- the pool's values of this class; n, min, max, arg-max
    float vals[kRowsPerThread];
    bool in_pool[kRowsPerThread];
    unsigned n_local = 0;
    float lo = 2.f, hi = -1.f;
    u64 amax = 0;
#pragma unroll
    for (int q = 0; q < kRowsPerThread; ++q) {
      const int r = t + q * kThreads;
      in_pool[q] = r < R && pool[r];
      vals[q] = in_pool[q] ? clip_prob(col[(size_t)r * ld_prev]) : 0.f;
      if (in_pool[q]) {
        ++n_local;
        lo = fminf(lo, vals[q]);
        hi = fmaxf(hi, vals[q]);
        amax = max(amax, index_key(__float_as_uint(vals[q]), (unsigned)r));   // (positive floats order as their bits)
      }
    }
    const int n = (int)wg_reduce((u64)n_local, Add(), slot_u);
    if (n == 0) continue;                                                    // (uniform)
    lo = wg_reduce(lo, Min(), slot_f);
    hi = wg_reduce(hi, Max(), slot_f);
    amax = wg_reduce(amax, Max(), slot_u);
    // ---- Lloyd
    const int nc = min(3, n);
    double ctr[3] = {(double)lo, nc == 3 ? ((double)lo + (double)hi) / 2.0 : (double)hi, (double)hi};
    int asg[kRowsPerThread];
#pragma unroll
    for (int q = 0; q < kRowsPerThread; ++q) asg[q] = -1;
    for (int pass = 0; pass < kLloydPasses && nc > 1; ++pass) {
      double s0 = 0.0, s1 = 0.0, s2 = 0.0;
      u64 packed = 0;                                // counts of the three clusters and of changed rows, 16 bits each
#pragma unroll
      for (int q = 0; q < kRowsPerThread; ++q) {
        if (!in_pool[q]) continue;
        const double v = (double)vals[q];
        int best = 0;
        double bd = fabs(v - ctr[0]);
        for (int k = 1; k < nc; ++k) {
          const double d = fabs(v - ctr[k]);
          if (d < bd) { bd = d; best = k; }          // strict: a tie stays with the lower centre
        }
        if (best != asg[q]) packed += 1ull << 48;
        asg[q] = best;
        if (best == 0) s0 += v; else if (best == 1) s1 += v; else s2 += v;
        packed += 1ull << (16 * best);
      }
      packed = wg_reduce(packed, Add(), slot_u);
      if ((packed >> 48) == 0) break;                // no assignment changed (uniform)
      s0 = wg_reduce(s0, Add(), slot_d);
      s1 = wg_reduce(s1, Add(), slot_d);
      s2 = wg_reduce(s2, Add(), slot_d);
      const unsigned n0 = packed & 0xFFFF, n1 = (packed >> 16) & 0xFFFF, n2 = (packed >> 32) & 0xFFFF;
      if (n0) ctr[0] = s0 / (double)n0;
      if (n1) ctr[1] = s1 / (double)n1;
      if (n2) ctr[2] = s2 / (double)n2;
    }
    int top = 0;
    for (int k = 1; k < nc; ++k)
      if (ctr[k] > ctr[top]) top = k;                // the first of equal centres
    // ---- the top-ranking set, ascending rows
    int T = 0;
#pragma unroll
    for (int q = 0; q < kRowsPerThread; ++q) {
      const bool member = in_pool[q] && (nc == 1 || asg[q] == top);
      int cnt;
      const int s = compact_wg<kThreads / 64>(member, wave_count, cnt);
      if (member) tlist[T + s] = (unsigned short)(t + q * kThreads);
      T += cnt;
    }
    if (T == 0) {                                    // an empty top cluster: the arg-max proposal
      if (t == 0) tlist[0] = (unsigned short)key_index(amax);
      T = 1;
    }
    __syncthreads();
    // ---- graph
    const int words = (T + 63) / 64;
    for (int item = t; item < T * words; item += kThreads) {
      const int a = item / words, wb = item - a * words;
      const float4 ba = load_box(boxes, off + tlist[a]);
      u64 bits = 0;
      const int b1 = min(64, T - wb * 64);
      for (int k = 0; k < b1; ++k) {
        const int b = wb * 64 + k;
        if (b == a || box_iou(ba, load_box(boxes, off + tlist[b])) > kGraphIou) bits |= 1ull << k;
      }
      adj[(size_t)a * words + wb] = bits;
    }
    for (int w = t; w < words; w += kThreads) {
      const int b1 = min(64, T - w * 64);
      alive[w] = b1 == 64 ? ~0ull : ((1ull << b1) - 1ull);
    }
    __syncthreads();
    // ---- greedy centres
    int count = T, nk = 0;
    do {
      u64 key = 0;
      for (int a = t; a < T; a += kThreads) {
        if (!((alive[a >> 6] >> (a & 63)) & 1ull)) continue;
        unsigned deg = 0;
        for (int w = 0; w < words; ++w) deg += __popcll(adj[(size_t)a * words + w] & alive[w]);
        key = max(key, index_key(deg, (unsigned)a));
      }
      key = wg_reduce(key, Max(), slot_u);
      const int deg = (int)(key >> 32);
      if (deg == 0) break;                           // (nothing left; with self edges only when count is 0)
      const int node = (int)key_index(key);
      float sc = 0.f;
      u64 nb = 0;
      if (t < words) {                               // words <= 128 < kThreads
        nb = adj[(size_t)node * words + t] & alive[t];
        for (u64 m = nb; m; m &= m - 1) {
          const int b = t * 64 + __builtin_ctzll(m);
          sc = fmaxf(sc, clip_prob(col[(size_t)tlist[b] * ld_prev]));
        }
      }
      sc = wg_reduce(sc, Max(), slot_f);            // (its barriers order the reads of alive above before the update)
      if (t < words) alive[t] &= ~nb;
      if (t == 0) { keep_node[nk] = node; keep_score[nk] = sc; }
      ++nk;
      count -= deg;
      __syncthreads();
    } while (count > 5);
    // ---- the best-scoring centres, at most 5, in descending order of score
    const int take = min(nk, kMaxPC);
    for (int s = 0; s < take; ++s) {
      u64 key = 0;
      for (int k = t; k < nk; k += kThreads) {
        const float v = keep_score[k];
        if (v > 0.f) key = max(key, index_key(__float_as_uint(v), (unsigned)k));
      }
      key = wg_reduce(key, Max(), slot_u);
      if (key == 0) break;
      const int k = (int)key_index(key);
      if (t == 0) {
        const int row = tlist[keep_node[k]];
        pci[G * 3 + 0] = c + 1;
        pci[G * 3 + 2] = row;
        pcf[G * 3 + 0] = keep_score[k];
        keep_score[k] = -1.f;                        // taken
        pool[row] = 0;                               // leaves the pool of the later classes
      }
      ++G;
      __syncthreads();
    }
  }
  if (t == 0) pc_num[img] = G;
}

// ---- every proposal to its highest-IoU centre: one thread per proposal
__global__ __launch_bounds__(256) void pcl_assign_kernel(const float* __restrict__ boxes, const int* __restrict__ offsets,
                                                         int nimg, int maxc, const int* __restrict__ pc_int,
                                                         const float* __restrict__ pc_flt, const int* __restrict__ pc_num,
                                                         int* __restrict__ row_label, int* __restrict__ row_assign,
                                                         float* __restrict__ row_weight) {
#pragma clang fp contract(off)
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= offsets[nimg]) return;
  const int img = image_of(offsets, nimg, r);
  const int off = offsets[img], G = pc_num[img];
  const int* __restrict__ pci = pc_int + (size_t)img * maxc * 3;
  const float* __restrict__ pcf = pc_flt + (size_t)img * maxc * 3;
  const float4 b = load_box(boxes, r);
  float best = -1.f;
  int bj = -1;
  for (int j = 0; j < G; ++j) {
    const float v = box_iou(b, load_box(boxes, off + pci[j * 3 + 2]));
    if (v > best) { best = v; bj = j; }               // strict: the first maximum
  }
  int label = 0, asg = -1;
  float w = 0.f;
  if (bj >= 0) {
    w = best < kBgIou ? 0.f : pcf[bj * 3 + 0];
    if (!(best < kFgIou)) { label = pci[bj * 3 + 0]; asg = bj; }
  }
  row_label[r] = label;
  row_assign[r] = asg;
  row_weight[r] = w;
}

// ---- per cluster: member count, summed weight, mean clipped probability.  grid (maxc, nimg), 256 threads.
__global__ __launch_bounds__(256) void pcl_stats_kernel(const float* __restrict__ probs, int ld_probs,
                                                        const int* __restrict__ offsets, int maxc,
                                                        const int* __restrict__ row_assign, int* __restrict__ pc_int,
                                                        float* __restrict__ pc_flt, const int* __restrict__ pc_num) {
#pragma clang fp contract(off)
  __shared__ double slot_d[4];
  __shared__ u64 slot_u[4];
  const int j = blockIdx.x, img = blockIdx.y;
  if (j >= pc_num[img]) return;                        // (uniform; the slot was zeroed by the centre search)
  int* __restrict__ pci = pc_int + ((size_t)img * maxc + j) * 3;
  float* __restrict__ pcf = pc_flt + ((size_t)img * maxc + j) * 3;
  const int cls = pci[0];
  const int off = offsets[img], end = offsets[img + 1];
  double sum = 0.0;
  u64 cnt = 0;
  for (int r = off + (int)threadIdx.x; r < end; r += 256)
    if (row_assign[r] == j) {
      ++cnt;
      sum += (double)clip_prob(probs[(size_t)r * ld_probs + cls]);
    }
  sum = wg_reduce(sum, Add(), slot_d);
  cnt = wg_reduce(cnt, Add(), slot_u);
  if (threadIdx.x == 0) {
    pci[1] = (int)cnt;
    pcf[1] = (float)((double)pcf[0] * (double)cnt);   // every member carries the centre's score
    pcf[2] = cnt ? (float)(sum / (double)cnt) : 0.f;
  }
}

// ---- row-wise soft-max, one thread per row
__global__ __launch_bounds__(256) void pcl_softmax_kernel(const float* __restrict__ z, int ld, int ncls, int R,
                                                          float* __restrict__ p) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const float* __restrict__ zr = z + (size_t)r * ld;
  float m = zr[0];
  for (int k = 1; k < ncls; ++k) m = fmaxf(m, zr[k]);
  float s = 0.f;
  for (int k = 0; k < ncls; ++k) s += expf(zr[k] - m);
  const float inv = 1.f / s;
  for (int k = 0; k < ncls; ++k) p[(size_t)r * ncls + k] = expf(zr[k] - m) * inv;
}

// ---- loss: one workgroup per image sums the background term and adds the cluster terms
__global__ __launch_bounds__(256) void pcl_loss_image_kernel(const float* __restrict__ probs, int ld_probs,
                                                             const int* __restrict__ offsets, int maxc,
                                                             const int* __restrict__ row_label,
                                                             const float* __restrict__ row_weight,
                                                             const int* __restrict__ pc_int,
                                                             const float* __restrict__ pc_flt,
                                                             const int* __restrict__ pc_num, double* __restrict__ per_image) {
  __shared__ double slot_d[4];
  const int img = blockIdx.x;
  const int off = offsets[img], end = offsets[img + 1];
  double bg = 0.0;
  for (int r = off + (int)threadIdx.x; r < end; r += 256)
    if (row_label[r] == 0) bg -= (double)row_weight[r] * log((double)fmaxf(probs[(size_t)r * ld_probs], 1e-6f));
  bg = wg_reduce(bg, Add(), slot_d);
  if (threadIdx.x == 0) {
    const int* __restrict__ pci = pc_int + (size_t)img * maxc * 3;
    const float* __restrict__ pcf = pc_flt + (size_t)img * maxc * 3;
    double l = bg;
    const int G = pc_num[img];
    for (int j = 0; j < G; ++j)
      if (pci[j * 3 + 1] > 0) l -= (double)pcf[j * 3 + 1] * log((double)fmaxf(pcf[j * 3 + 2], 1e-6f));
    per_image[img] = end > off ? l / (double)(end - off) : 0.0;
  }
}

__global__ void pcl_loss_finish_kernel(const double* __restrict__ per_image, int nimg, float* __restrict__ loss) {
  if (threadIdx.x || blockIdx.x) return;
  double s = 0.0;
  for (int i = 0; i < nimg; ++i) s += per_image[i];
  loss[0] = (float)(s / (double)max(nimg, 1));
}

// ---- gradient to the logits: one thread per row
__global__ __launch_bounds__(256) void pcl_backward_kernel(const float* __restrict__ z, int ld, int ncls,
                                                           const int* __restrict__ offsets, int nimg, int maxc,
                                                           const int* __restrict__ row_label,
                                                           const int* __restrict__ row_assign,
                                                           const float* __restrict__ row_weight,
                                                           const int* __restrict__ pc_int, const float* __restrict__ pc_flt,
                                                           const float* __restrict__ upstream, float* __restrict__ dz,
                                                           int ld_dz) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= offsets[nimg]) return;
  const int img = image_of(offsets, nimg, r);
  const int rows = offsets[img + 1] - offsets[img];
  const float* __restrict__ zr = z + (size_t)r * ld;
  float m = zr[0];
  for (int k = 1; k < ncls; ++k) m = fmaxf(m, zr[k]);
  float s = 0.f;
  for (int k = 0; k < ncls; ++k) s += expf(zr[k] - m);
  const float inv = 1.f / s;
  const int label = row_label[r];
  const float pstar = expf(zr[label] - m) * inv;
  float g;                                            // d loss_image / d p[r, label], before the 1 / R_i
  if (label == 0) {
    g = -row_weight[r] / fmaxf(pstar, 1e-5f);
  } else {
    const size_t j = ((size_t)img * maxc + row_assign[r]) * 3;
    g = -pc_flt[j + 1] / fmaxf((float)pc_int[j + 1] * pc_flt[j + 2], 1e-5f);
  }
  g *= (upstream ? upstream[0] : 1.f) / ((float)rows * (float)nimg);
  const float gp = g * pstar;                         // dz_k = g p* ([k == label] - p_k)
  for (int k = 0; k < ncls; ++k) {
    const float pk = expf(zr[k] - m) * inv;
    dz[(size_t)r * ld_dz + k] = gp * ((k == label ? 1.f : 0.f) - pk);
  }
}

// adj (nimg, rows, words) adjacency bits | keep_node (nimg, rows) | keep_score (nimg, rows), in 16-byte pieces
struct ClusterWs { u64* adj; int* keep_node; float* keep_score; };
ClusterWs carve(Arena& a, int nimg, int rows) {
  const size_t words = ((size_t)rows + 63) / 64;
  ClusterWs k;
  k.adj = a.take<u64>((size_t)nimg * rows * words);
  k.keep_node = a.take<int>((size_t)nimg * rows);
  k.keep_score = a.take<float>((size_t)nimg * rows);
  return k;
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" {

size_t jtsm_pcl_cluster_workspace_bytes(int nimg, int max_rows) {
  if (nimg <= 0 || max_rows <= 0) return 16;
  Arena a{nullptr, false, 16};
  carve(a, nimg, max_rows);
  return a.off;
}

int jtsm_pcl_cluster_f32(const float* boxes, const int32_t* offsets, int nimg, int max_rows, int total_rows,
                         const float* prev_probs, int ld_prev, int prev_col0, const float* labels, int num_classes,
                         const float* probs, int ld_probs, int32_t* row_label, int32_t* row_assign, float* row_weight,
                         int32_t* pc_int, float* pc_flt, int32_t* pc_num, void* workspace, void* stream) {
  JTSM_REQUIRE(nimg >= 0 && max_rows >= 0 && total_rows >= 0 && num_classes > 0, "pcl_cluster: negative size");
  JTSM_REQUIRE(max_rows <= kMaxRows, "pcl_cluster: at most %d proposals per image, got %d", kMaxRows, max_rows);
  JTSM_REQUIRE((long)nimg * max_rows >= total_rows, "pcl_cluster: max_rows %d too small for %d rows of %d images",
               max_rows, total_rows, nimg);
  if (nimg == 0) return JTSM_OK;
  JTSM_REQUIRE(offsets && labels && pc_int && pc_flt && pc_num && workspace, "pcl_cluster: null pointer");
  JTSM_REQUIRE(total_rows == 0 || (boxes && prev_probs && probs && row_label && row_assign && row_weight),
               "pcl_cluster: null pointer");
  JTSM_REQUIRE(ld_prev >= prev_col0 + num_classes && prev_col0 >= 0 && ld_probs >= num_classes + 1,
               "pcl_cluster: leading dimensions");
  JTSM_REQUIRE(((uintptr_t)boxes & 15) == 0 && ((uintptr_t)workspace & 15) == 0,
               "pcl_cluster: boxes and workspace must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const int maxc = kMaxPC * num_classes;
  const int rows_ws = std::max(max_rows, 1);
  Arena arena{static_cast<char*>(workspace), false, 16};
  const ClusterWs k = carve(arena, nimg, rows_ws);
  hipLaunchKernelGGL(pcl_centres_kernel, dim3(nimg), dim3(kThreads), 0, st, boxes, offsets, prev_probs, ld_prev, prev_col0,
                     labels, num_classes, maxc, rows_ws, k.adj, k.keep_node, k.keep_score, pc_int, pc_flt, pc_num);
  if (total_rows > 0)
    hipLaunchKernelGGL(pcl_assign_kernel, dim3(ceil_div(total_rows, 256)), dim3(256), 0, st, boxes, offsets, nimg, maxc,
                       pc_int, pc_flt, pc_num, row_label, row_assign, row_weight);
  hipLaunchKernelGGL(pcl_stats_kernel, dim3(maxc, nimg), dim3(256), 0, st, probs, ld_probs, offsets, maxc, row_assign,
                     pc_int, pc_flt, pc_num);
  JTSM_CHECK_LAUNCH("pcl_cluster");
  return JTSM_OK;
}

int jtsm_pcl_softmax_f32(const float* logits, int ld, int num_cls, int R, float* probs, void* stream) {
  JTSM_REQUIRE(R >= 0 && num_cls > 0 && ld >= num_cls, "pcl_softmax: bad sizes");
  if (R == 0) return JTSM_OK;
  JTSM_REQUIRE(logits && probs, "pcl_softmax: null pointer");
  hipLaunchKernelGGL(pcl_softmax_kernel, dim3(ceil_div(R, 256)), dim3(256), 0, as_stream(stream), logits, ld, num_cls, R,
                     probs);
  JTSM_CHECK_LAUNCH("pcl_softmax");
  return JTSM_OK;
}

size_t jtsm_pcl_loss_workspace_bytes(int nimg) {
  Arena a{nullptr, false, 16};
  a.take<double>((size_t)std::max(nimg, 1));   // per_image
  return a.off;
}

int jtsm_pcl_loss_forward_f32(const float* probs, int ld_probs, const int32_t* offsets, int nimg, int num_classes,
                              const int32_t* row_label, const float* row_weight, const int32_t* pc_int,
                              const float* pc_flt, const int32_t* pc_num, float* loss, void* workspace, void* stream) {
  JTSM_REQUIRE(nimg >= 0 && num_classes > 0 && ld_probs >= num_classes + 1, "pcl_loss: bad sizes");
  JTSM_REQUIRE(loss && workspace, "pcl_loss: null pointer");
  JTSM_REQUIRE(nimg == 0 || (offsets && pc_int && pc_flt && pc_num), "pcl_loss: null pointer");
  hipStream_t st = as_stream(stream);
  double* per_image = reinterpret_cast<double*>(workspace);
  if (nimg > 0)
    hipLaunchKernelGGL(pcl_loss_image_kernel, dim3(nimg), dim3(256), 0, st, probs, ld_probs, offsets,
                       kMaxPC * num_classes, row_label, row_weight, pc_int, pc_flt, pc_num, per_image);
  hipLaunchKernelGGL(pcl_loss_finish_kernel, dim3(1), dim3(64), 0, st, per_image, nimg, loss);
  JTSM_CHECK_LAUNCH("pcl_loss forward");
  return JTSM_OK;
}

int jtsm_pcl_loss_backward_f32(const float* logits, int ld, int num_classes, const int32_t* offsets, int nimg,
                               int total_rows, const int32_t* row_label, const int32_t* row_assign,
                               const float* row_weight, const int32_t* pc_int, const float* pc_flt,
                               const float* upstream, float* d_logits, int ld_grad, void* stream) {
  JTSM_REQUIRE(nimg >= 0 && total_rows >= 0 && num_classes > 0 && ld >= num_classes + 1 && ld_grad >= num_classes + 1,
               "pcl_loss backward: bad sizes");
  if (total_rows == 0 || nimg == 0) return JTSM_OK;
  JTSM_REQUIRE(logits && offsets && row_label && row_assign && row_weight && pc_int && pc_flt && d_logits,
               "pcl_loss backward: null pointer");
  hipLaunchKernelGGL(pcl_backward_kernel, dim3(ceil_div(total_rows, 256)), dim3(256), 0, as_stream(stream), logits, ld,
                     num_classes + 1, offsets, nimg, kMaxPC * num_classes, row_label, row_assign, row_weight, pc_int,
                     pc_flt, upstream, d_logits, ld_grad);
  JTSM_CHECK_LAUNCH("pcl_loss backward");
  return JTSM_OK;
}

}  // extern "C"
