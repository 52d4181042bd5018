// Panoptic quality and the semantic confusion matrix on the device: the arithmetic behind the reference's
// COCOPanopticEvaluator (detectron2/evaluation/panoptic_evaluation.py:66-144 — PNG files, then panopticapi's
// pq_compute_single_core) and SemSegEvaluator.process (sem_seg_evaluation.py:82-93 — one np.bincount per image) on the
// maps where inference left them.  Semantics: DESIGN.md §4f.
//
//   jtsm_pq_accumulate, one image per call:
//     lookup   pred_table's ids into an open-addressing table (the smallest row wins a duplicated id);
//     hist     the (G+1) x (P+1) pair histogram I[g][p], index 0 = VOID on either side: per-workgroup LDS counters
//              flushed with integer atomics while the table fits kPqLdsCells, global atomics above; 16-byte loads of
//              both maps, four pixels per thread, one atomic per wavefront where all its pixels fall into one cell;
//     finish   one workgroup: counted areas (row / column sums), the IoU > 0.5 matches (unique per row and per column,
//              so no order is involved), fn / fp / tp as integer atomics, then ONE thread adds the matched IoUs to
//              iou_sum in gt-row order — plain fp64 adds, bit-reproducible.
//   jtsm_confusion_accumulate: the (C+1)^2 histogram the same way.
//
// Integer arithmetic throughout but `iou = I / union`, `x / area > 0.5` and `iou_sum += iou`: one correctly rounded
// operation each, nothing a contraction could fuse — no per-file build flag.
#include <climits>

#include "common.h"
#include "workspace.h"

namespace jtsm {
namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

// LDS per CU is 160 KiB and two workgroups of 1024 threads fill a CU's 32 wavefront slots: a workgroup may take 80 KiB
// without costing occupancy — 64 KiB of counters and, for the pair histogram, 16 KiB of id lookup.
constexpr int kPqLdsCells = 16384;      // int32 counters of the pair histogram in LDS: (G+1)(P+1) at most this
constexpr int kConfLdsCells = 16384;    // int32 counters of the confusion matrix in LDS: (C+1)^2 at most this, C <= 127
constexpr int kLdsHash = 2048;          // id lookup slots in LDS (key + row): P + 1 <= 1024
constexpr int kThreads = 1024;
constexpr int kMaxBlocks = 512;
constexpr long kMaxCells = 1L << 28;

__host__ __device__ inline int hash_slots(int P) {   // a power of two >= 2 (P + 1), at least 64
  int s = 64;
  while (s < 2 * (P + 1)) s <<= 1;
  return s;
}
__device__ __forceinline__ u32 hash_of(int id, int mask) { return ((u32)id * 2654435761u >> 7) & (u32)mask; }

// keys / vals zeroed by the caller; val = P - row, so the largest value is the smallest row (0 = empty)
__global__ __launch_bounds__(256) void pq_lookup_kernel(const int* __restrict__ pred_table,
                                                        const int* __restrict__ num_pred, int P, int mask,
                                                        int* __restrict__ keys, int* __restrict__ vals) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= min(max(*num_pred, 0), P)) return;
  const int id = pred_table[5 * r];
  if (id == 0) return;                                 // 0 is VOID: such a row can own no pixel
  u32 s = hash_of(id, mask);
  for (;;) {                                           // at most half the slots are ever taken
    const int was = atomicCAS(&keys[s], 0, id);
    if (was == 0 || was == id) break;
    s = (s + 1) & (u32)mask;
  }
  atomicMax(&vals[s], P - r);
}

// row + 1 of a predicted id, 0 (VOID) for 0 and for an id in no row (then counted in `bad`)
__device__ __forceinline__ int lookup(int id, const int* keys, const int* vals, int mask, int P, int& last_id,
                                      int& last_p, int& bad) {
  if (id == last_id) return last_p;
  int p = 0;
  if (id != 0) {
    u32 s = hash_of(id, mask);
    for (;;) {
      const int k = keys[s];
      if (k == id) { p = P - vals[s] + 1; break; }
      if (k == 0) { ++bad; return 0; }                 // (not remembered: every such pixel is counted)
      s = (s + 1) & (u32)mask;
    }
  }
  last_id = id;
  last_p = p;
  return p;
}

template <typename T>
__device__ __forceinline__ void bump(T* h, long cell, int by) { atomicAdd(&h[cell], (T)by); }

// Adds `cnt` to h[cell] for every lane that is `in`; called in wave-uniform control flow.  Where all those lanes
// name one cell with one count (the inside of a segment), lane 0 adds for the wavefront.
template <typename T>
__device__ __forceinline__ void wave_bump(T* h, bool in, int cell, int cnt) {
  const u64 m_in = __ballot(in);
  const int lead = __builtin_amdgcn_readfirstlane(cell), lead_cnt = __builtin_amdgcn_readfirstlane(cnt);
  const u64 m_same = __ballot(in && cell == lead && cnt == lead_cnt);
  if ((m_in & 1ull) && m_same == m_in) {               // (lane 0 is `in`: lead is a real cell)
    if ((threadIdx.x & 63) == 0) bump(h, lead, lead_cnt * __popcll(m_in));
  } else if (in) {
    bump(h, cell, cnt);
  }
}

// nvec: number of 4-pixel groups read as int4 (0 when an address is not 16-byte aligned); the rest is read singly.
template <bool HIST_LDS, bool HASH_LDS>
__global__ __launch_bounds__(kThreads) void pq_hist_kernel(const int* __restrict__ pred, const int* __restrict__ gt,
                                                           long n, long nvec, int G, int P, int cells,
                                                           const int* __restrict__ gkeys,
                                                           const int* __restrict__ gvals, int mask,
                                                           int* __restrict__ hist, u64* __restrict__ stats) {
  __shared__ int sh_hist[HIST_LDS ? kPqLdsCells : 1];
  __shared__ int sh_keys[HASH_LDS ? kLdsHash : 1];
  __shared__ int sh_vals[HASH_LDS ? kLdsHash : 1];
  const int tid = threadIdx.x, P1 = P + 1;
  if (HIST_LDS)
    for (int c = tid; c < cells; c += kThreads) sh_hist[c] = 0;
  if (HASH_LDS)
    for (int s = tid; s <= mask; s += kThreads) { sh_keys[s] = gkeys[s]; sh_vals[s] = gvals[s]; }
  if (HIST_LDS || HASH_LDS) __syncthreads();
  int* h = HIST_LDS ? sh_hist : hist;
  const int* keys = HASH_LDS ? sh_keys : gkeys;
  const int* vals = HASH_LDS ? sh_vals : gvals;
  int last_id = 0, last_p = 0, bad = 0;
  auto cell_of = [&](int gv, int pv) {
    if (gv < 0 || gv > G) { ++bad; gv = 0; }
    return gv * P1 + lookup(pv, keys, vals, mask, P, last_id, last_p, bad);
  };

  const int4* pred4 = reinterpret_cast<const int4*>(pred);
  const int4* gt4 = reinterpret_cast<const int4*>(gt);
  const long stride = (long)gridDim.x * kThreads;
  for (long base = (long)blockIdx.x * kThreads; base < nvec; base += stride) {        // (block-uniform)
    const long i = base + tid;
    const bool in = i < nvec;
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    if (in) {
      const int4 a = pred4[i], b = gt4[i];
      c0 = cell_of(b.x, a.x); c1 = cell_of(b.y, a.y); c2 = cell_of(b.z, a.z); c3 = cell_of(b.w, a.w);
    }
    const bool one = c0 == c1 && c0 == c2 && c0 == c3;
    if (__all(!in || one)) {
      wave_bump(h, in, c0, 4);
    } else if (in) {
      if (one) bump(h, c0, 4);
      else { bump(h, c0, 1); bump(h, c1, 1); bump(h, c2, 1); bump(h, c3, 1); }
    }
  }
  for (long base = nvec * 4 + (long)blockIdx.x * kThreads; base < n; base += stride) {
    const long i = base + tid;
    const bool in = i < n;
    const int c = in ? cell_of(gt[i], pred[i]) : 0;
    wave_bump(h, in, c, 1);
  }

  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
  if ((tid & 63) == 0 && bad) atomicAdd(&stats[0], (u64)bad);
  if (HIST_LDS) {
    __syncthreads();
    for (int c = tid; c < cells; c += kThreads) {
      const int v = sh_hist[c];
      if (v) atomicAdd(&hist[c], v);
    }
  }
}

struct PqWs {
  size_t zeroed, zeroed_end;        // arena marks around hist .. crowd_row: cleared by one memset
  int *hist, *keys, *vals, *pmatched, *crowd_row;
  int *pcat, *area_p, *match_p;
  double* iou;
  int slots;
};

PqWs carve(Arena& a, int G, int P, int C) {
  const size_t g1 = (size_t)(G > 0 ? G : 0) + 1, p1 = (size_t)(P > 0 ? P : 0) + 1, c = C > 0 ? C : 1;
  PqWs w;
  w.slots = hash_slots(P > 0 ? P : 0);
  w.zeroed = a.mark();
  w.hist = a.take<int>(g1 * p1);
  w.keys = a.take<int>(w.slots);
  w.vals = a.take<int>(w.slots);
  w.pmatched = a.take<int>(p1);
  w.crowd_row = a.take<int>(c);
  w.zeroed_end = a.mark();
  w.pcat = a.take<int>(p1);
  w.area_p = a.take<int>(p1);
  w.match_p = a.take<int>(g1);
  w.iou = a.take<double>(g1);
  return w;
}

// One workgroup.  hist is complete (the stream orders the launches); everything else here is this workgroup's own.
__global__ __launch_bounds__(kThreads) void pq_finish_kernel(
    const int* __restrict__ hist, const int* __restrict__ pred_table, const int* __restrict__ num_pred, int P,
    const int* __restrict__ thing_cat, int num_things, const int* __restrict__ stuff_cat, int num_stuff,
    const int* __restrict__ gt_table, int G, int C, int* pcat, int* area_p, int* pmatched, int* crowd_row,
    int* match_p, double* iou_g, u64* tp, u64* fp, u64* fn, double* iou_sum, u64* stats) {
  __shared__ int sh_cat[kThreads];
  __shared__ double sh_iou[kThreads];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, P1 = P + 1;
  const int np = min(max(P > 0 ? *num_pred : 0, 0), P);
  // evaluation category of gt row g (1-based): -1 = left out
  auto gcat_of = [&](int g) { const int c = gt_table[2 * (g - 1)]; return (c >= 0 && c < C) ? c : -1; };

  // A: per predicted row its category (-2: beyond num_pred) and counted area; per category its last crowd row
  for (int p = 1 + tid; p <= P; p += kThreads) {
    int cat = -2;
    if (p - 1 < np) {
      const int isthing = pred_table[5 * (p - 1) + 1], k = pred_table[5 * (p - 1) + 2];
      cat = isthing ? ((k >= 0 && k < num_things) ? thing_cat[k] : -1) : ((k >= 0 && k < num_stuff) ? stuff_cat[k] : -1);
      if (cat < 0 || cat >= C) { cat = -1; atomicAdd(&stats[2], 1ull); }
    }
    pcat[p] = cat;
    int a = 0;
    for (int g = 0; g <= G; ++g) a += hist[(long)g * P1 + p];
    area_p[p] = a;
    if (cat != -2 && a == 0) atomicAdd(&stats[1], 1ull);
  }
  for (int g = 1 + tid; g <= G; g += kThreads) {
    const int cat = gcat_of(g);
    if (cat < 0) atomicAdd(&stats[2], 1ull);
    else if (gt_table[2 * (g - 1) + 1] != 0) atomicMax(&crowd_row[cat], g);
  }
  __syncthreads();

  // B: one wavefront per gt row: its area, then the one predicted row (if any) with IoU > 0.5
  for (int g = 1 + wv; g <= G; g += kThreads / 64) {
    const int* row = hist + (long)g * P1;
    const int cat = gcat_of(g);
    const bool live = cat >= 0 && gt_table[2 * (g - 1) + 1] == 0;      // (wave-uniform)
    int found = 0;
    if (live) {
      int area_g = 0;
      for (int p = lane; p <= P; p += 64) area_g += row[p];
      for (int o = 32; o > 0; o >>= 1) area_g += __shfl_xor(area_g, o);
      for (int p = 1 + lane; p <= P; p += 64) {
        const int v = row[p];
        if (v > 0 && pcat[p] == cat) {
          const long long uni = (long long)area_p[p] + area_g - v - hist[p];
          const double iou = (double)v / (double)uni;
          if (iou > 0.5) { found = p; iou_g[g] = iou; pmatched[p] = 1; }
        }
      }
      for (int o = 32; o > 0; o >>= 1) found = max(found, __shfl_xor(found, o));
    }
    if (lane == 0) {
      match_p[g] = found;
      if (live) atomicAdd(found ? &tp[cat] : &fn[cat], 1ull);
    }
  }
  __syncthreads();

  // C: unmatched predicted rows are false positives unless more than half of them lies on VOID and the crowd row
  for (int p = 1 + tid; p <= P; p += kThreads) {
    const int cat = pcat[p];
    if (cat < 0 || pmatched[p]) continue;
    long long x = hist[p];
    const int k = crowd_row[cat];
    if (k) x += hist[(long)k * P1 + p];
    if (!((double)x / (double)area_p[p] > 0.5)) atomicAdd(&fp[cat], 1ull);
  }

  // D: the matched IoUs in gt-row order, added by one thread
  for (int g0 = 1; g0 <= G; g0 += kThreads) {
    const int g = g0 + tid;
    int cat = -1;
    if (g <= G && match_p[g]) { cat = gcat_of(g); sh_iou[tid] = iou_g[g]; }
    sh_cat[tid] = cat;
    __syncthreads();
    if (tid == 0) {
      const int m = min(kThreads, G - g0 + 1);
      for (int j = 0; j < m; ++j)
        if (sh_cat[j] >= 0) iou_sum[sh_cat[j]] = iou_sum[sh_cat[j]] + sh_iou[j];
    }
    __syncthreads();
  }
  if (tid == 0) atomicAdd(&stats[3], 1ull);
}

// ---------------------------------------------------------------------------------------------------- confusion
template <typename GT> struct Vec4;
template <> struct Vec4<unsigned char> { typedef uchar4 type; };
template <> struct Vec4<int> { typedef int4 type; };

template <typename GT, bool LDS>
__global__ __launch_bounds__(kThreads) void confusion_kernel(const long long* __restrict__ pred,
                                                             const GT* __restrict__ gt, long n, long nvec, int C,
                                                             int ignore_label, u64* __restrict__ conf,
                                                             u64* __restrict__ stats) {
  __shared__ int sh[LDS ? kConfLdsCells : 1];
  typedef typename Vec4<GT>::type GT4;
  const int tid = threadIdx.x, C1 = C + 1, cells = C1 * C1;
  if (LDS) {
    for (int c = tid; c < cells; c += kThreads) sh[c] = 0;
    __syncthreads();
  }
  int bad = 0;
  auto cell_of = [&](long long p, int g) {             // -1: left out
    if (g == ignore_label) g = C;
    if (p < 0 || p >= C || g < 0 || g > C) { ++bad; return -1; }
    return (int)p * C1 + g;
  };
  auto add = [&](bool in, int cell) {
    if (LDS) wave_bump(sh, in && cell >= 0, cell, 1);
    else wave_bump(conf, in && cell >= 0, cell, 1);
  };
  const longlong2* pred2 = reinterpret_cast<const longlong2*>(pred);
  const GT4* gt4 = reinterpret_cast<const GT4*>(gt);
  const long stride = (long)gridDim.x * kThreads;
  for (long base = (long)blockIdx.x * kThreads; base < nvec; base += stride) {        // (block-uniform)
    const long i = base + tid;
    const bool in = i < nvec;
    int c0 = -1, c1 = -1, c2 = -1, c3 = -1;
    if (in) {
      const longlong2 a = pred2[2 * i], b = pred2[2 * i + 1];
      const GT4 g = gt4[i];
      c0 = cell_of(a.x, (int)g.x); c1 = cell_of(a.y, (int)g.y); c2 = cell_of(b.x, (int)g.z); c3 = cell_of(b.y, (int)g.w);
    }
    add(in, c0); add(in, c1); add(in, c2); add(in, c3);
  }
  for (long base = nvec * 4 + (long)blockIdx.x * kThreads; base < n; base += stride) {
    const long i = base + tid;
    const bool in = i < n;
    add(in, in ? cell_of(pred[i], (int)gt[i]) : -1);
  }
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
  if ((tid & 63) == 0 && bad) atomicAdd(&stats[0], (u64)bad);
  if (LDS) {
    __syncthreads();
    for (int c = tid; c < cells; c += kThreads) {
      const int v = sh[c];
      if (v) atomicAdd(&conf[c], (u64)v);
    }
  }
}

inline int hist_blocks(long nvec, long n) {
  const long work = nvec > 0 ? nvec : n;
  const long b = (work + kThreads - 1) / kThreads;
  return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" int jtsm_pq_lds_cells(void) { return kPqLdsCells; }
extern "C" int jtsm_confusion_lds_cells(void) { return kConfLdsCells; }

extern "C" size_t jtsm_pq_accumulate_workspace_bytes(int G, int P, int C) {
  if ((long)((G > 0 ? G : 0) + 1L) * ((P > 0 ? P : 0) + 1L) > kMaxCells) return 0;
  Arena a{nullptr};
  carve(a, G, P, C);
  return a.off;
}

extern "C" int jtsm_pq_accumulate(const int32_t* pred, const int32_t* pred_table, const int32_t* num_pred, int P,
                                  const int32_t* thing_cat, int num_things, const int32_t* stuff_cat, int num_stuff,
                                  const int32_t* gt, const int32_t* gt_table, int G, long pixels, int C, int64_t* tp,
                                  int64_t* fp, int64_t* fn, double* iou_sum, int64_t* stats, int force_global,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  JTSM_REQUIRE(G >= 0 && P >= 0 && C >= 1 && pixels >= 0 && pixels <= INT_MAX && num_things >= 0 && num_stuff >= 0,
               "pq_accumulate: G=%d P=%d C=%d pixels=%ld num_things=%d num_stuff=%d", G, P, C, pixels, num_things,
               num_stuff);
  const long cells = (G + 1L) * (P + 1L);
  JTSM_REQUIRE(cells <= kMaxCells, "pq_accumulate: (G+1)(P+1) = %ld exceeds %ld", cells, kMaxCells);
  JTSM_REQUIRE(tp && fp && fn && iou_sum && stats, "pq_accumulate: null totals");
  JTSM_REQUIRE(pixels == 0 || (pred && gt), "pq_accumulate: null map");
  JTSM_REQUIRE(P == 0 || (pred_table && num_pred), "pq_accumulate: null pred_table / num_pred");
  JTSM_REQUIRE(G == 0 || gt_table, "pq_accumulate: null gt_table");
  JTSM_REQUIRE((num_things == 0 || thing_cat) && (num_stuff == 0 || stuff_cat), "pq_accumulate: null category map");
  Arena arena{static_cast<char*>(workspace)};
  const PqWs w = carve(arena, G, P, C);
  JTSM_REQUIRE(workspace && workspace_bytes >= arena.off && ((size_t)workspace & 255) == 0,
               "pq_accumulate: workspace of %zu bytes (256-byte aligned) needed", arena.off);
  hipStream_t st = as_stream(stream);
  u64* st64 = reinterpret_cast<u64*>(stats);
  const int mask = w.slots - 1;

  JTSM_CHECK_HIP(hipMemsetAsync(arena.base + w.zeroed, 0, w.zeroed_end - w.zeroed, st));
  if (P > 0) {
    hipLaunchKernelGGL(pq_lookup_kernel, dim3(ceil_div(P, 256)), dim3(256), 0, st, pred_table, num_pred, P, mask,
                       w.keys, w.vals);
    JTSM_CHECK_LAUNCH("pq lookup");
  }
  if (pixels > 0) {
    const bool aligned = (((size_t)pred | (size_t)gt) & 15) == 0;
    const long nvec = aligned ? pixels / 4 : 0;
    const bool hist_lds = !force_global && cells <= kPqLdsCells, hash_lds = w.slots <= kLdsHash;
    const dim3 grid(hist_blocks(nvec, pixels)), block(kThreads);
#define JTSM_PQ_HIST(A, B)                                                                                         \
  hipLaunchKernelGGL((pq_hist_kernel<A, B>), grid, block, 0, st, pred, gt, pixels, nvec, G, P, (int)cells, w.keys, \
                     w.vals, mask, w.hist, st64)
    if (hist_lds && hash_lds) JTSM_PQ_HIST(true, true);
    else if (hist_lds) JTSM_PQ_HIST(true, false);
    else if (hash_lds) JTSM_PQ_HIST(false, true);
    else JTSM_PQ_HIST(false, false);
#undef JTSM_PQ_HIST
    JTSM_CHECK_LAUNCH("pq hist");
  }
  hipLaunchKernelGGL(pq_finish_kernel, dim3(1), dim3(kThreads), 0, st, w.hist, pred_table, num_pred, P, thing_cat,
                     num_things, stuff_cat, num_stuff, gt_table, G, C, w.pcat, w.area_p, w.pmatched, w.crowd_row,
                     w.match_p, w.iou, reinterpret_cast<u64*>(tp), reinterpret_cast<u64*>(fp),
                     reinterpret_cast<u64*>(fn), iou_sum, st64);
  JTSM_CHECK_LAUNCH("pq finish");
  return JTSM_OK;
}

extern "C" int jtsm_confusion_accumulate(const int64_t* pred, const void* gt, int gt_elem_bytes, long pixels,
                                         int num_classes, int ignore_label, int64_t* conf, int64_t* stats,
                                         int force_global, void* stream) {
  JTSM_REQUIRE(num_classes >= 1 && num_classes < 32768 && pixels >= 0 && pixels <= INT_MAX,
               "confusion_accumulate: num_classes=%d pixels=%ld", num_classes, pixels);
  JTSM_REQUIRE(gt_elem_bytes == 1 || gt_elem_bytes == 4, "confusion_accumulate: gt_elem_bytes=%d (1 or 4)",
               gt_elem_bytes);
  JTSM_REQUIRE(conf && stats, "confusion_accumulate: null conf / stats");
  if (pixels == 0) return JTSM_OK;
  JTSM_REQUIRE(pred && gt, "confusion_accumulate: null map");
  JTSM_REQUIRE(((size_t)pred & 7) == 0 && ((size_t)gt & (size_t)(gt_elem_bytes - 1)) == 0,
               "confusion_accumulate: misaligned map");
  const long cells = (num_classes + 1L) * (num_classes + 1L);
  const bool lds = !force_global && cells <= kConfLdsCells;
  const bool aligned = ((size_t)pred & 15) == 0 && ((size_t)gt & (size_t)(4 * gt_elem_bytes - 1)) == 0;
  const long nvec = aligned ? pixels / 4 : 0;
  const dim3 grid(hist_blocks(nvec, pixels)), block(kThreads);
  hipStream_t st = as_stream(stream);
  const long long* p = reinterpret_cast<const long long*>(pred);
  u64* c64 = reinterpret_cast<u64*>(conf);
  u64* s64 = reinterpret_cast<u64*>(stats);
#define JTSM_CONF(T, L)                                                                                            \
  hipLaunchKernelGGL((confusion_kernel<T, L>), grid, block, 0, st, p, static_cast<const T*>(gt), pixels, nvec,     \
                     num_classes, ignore_label, c64, s64)
  if (gt_elem_bytes == 1) { if (lds) JTSM_CONF(unsigned char, true); else JTSM_CONF(unsigned char, false); }
  else { if (lds) JTSM_CONF(int, true); else JTSM_CONF(int, false); }
#undef JTSM_CONF
  JTSM_CHECK_LAUNCH("confusion");
  return JTSM_OK;
}
