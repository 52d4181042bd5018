// RetinaNet on the device: anchor labelling, the focal / smooth-L1 losses with their normaliser each way,
// and the per-level candidate selection and decode of inference.  Built with -ffp-contract=off: a label is an integer
// decided by an IoU compared with the thresholds and with a per-gt maximum, so the IoU must have the reference's bits.
//
// The head's outputs are read where the convolutions wrote them.  A level's map is channels-last: per image `cells`
// = H * W cells, `cell_stride` floats apart, each holding A rows of K (logits) or 4 (deltas) floats back to back; the
// floats of a cell beyond A * K are padding (conv2d_padded).  Row r = cell * A + a of level l is anchor
// anchor_offset[l] + r.  A plain (N, HWA, K) tensor with a row stride is the case A = 1.
//
// No float atomics: every float sum has a fixed order (per-workgroup fp64 partials, one final pass).  The integer
// atomics (a max over non-negative float bits, counters, histogram bins) are order-free.
#include "box_math.h"
#include "common.h"
#include "reduce.h"
#include "workspace.h"

#include <cmath>
#include <cstring>

namespace jtsm {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxLevels = 8;
constexpr int kMaxThresholds = 8;
constexpr int kChunk = 256;            // gt boxes staged in LDS at a time
constexpr int kBins = 65536;           // one 16-bit digit of the selection key
constexpr int kSelectThreads = 1024;
constexpr int kMaxGrid = 4096;

typedef unsigned long long u64;

// ---- the level table -----------------------------------------------------------------------------------------------
struct Level {
  const float* x;      // logits (or their gradient)
  const float* d;      // deltas (or their gradient)
  long x_img, d_img;   // image strides, floats
  int cells, off;      // H * W; first anchor row in R
  int x_cell, d_cell;  // cell strides, floats
  int upc;             // work units per cell of the kernel being launched
  long unit0;          // first unit of the level
};
struct Table {
  Level lv[kMaxLevels];
  int L;
  long units;
};

// geom: L rows of 6 = cells, anchor_offset, logits image stride, logits cell stride, deltas image stride, deltas cell stride
int fill_table(Table& T, const float* const* logits, const float* const* deltas, const int64_t* geom, int L, int N,
               int A, int K, long R, const char* what) {
  JTSM_REQUIRE(L >= 1 && L <= kMaxLevels, "%s: %d levels (1..%d)", what, L, kMaxLevels);
  JTSM_REQUIRE(N >= 0 && A >= 1 && K >= 1 && (long)A * K < (1L << 24), "%s: N=%d A=%d K=%d", what, N, A, K);
  JTSM_REQUIRE(geom, "%s: null geometry", what);
  T.L = L;
  long rows = 0;
  for (int l = 0; l < L; ++l) {
    Level& v = T.lv[l];
    const int64_t* g = geom + 6 * l;
    v.x = logits ? logits[l] : nullptr;
    v.d = deltas ? deltas[l] : nullptr;
    JTSM_REQUIRE(g[0] >= 0 && g[0] * A < (1L << 31) / K, "%s: level %d has %ld cells", what, l, (long)g[0]);
    v.cells = (int)g[0];
    v.off = (int)g[1];
    JTSM_REQUIRE(g[1] == rows, "%s: level %d starts at anchor %ld, expected %ld", what, l, (long)g[1], rows);
    rows += (long)v.cells * A;
    v.x_img = g[2];
    v.d_img = g[4];
    JTSM_REQUIRE(g[3] >= (long)A * K && g[3] < (1L << 30) && g[5] >= 4L * A && g[5] < (1L << 30),
                 "%s: level %d cell strides %ld / %ld for A=%d K=%d", what, l, (long)g[3], (long)g[5], A, K);
    v.x_cell = (int)g[3];
    v.d_cell = (int)g[5];
    JTSM_REQUIRE(v.x_img >= (long)v.cells * v.x_cell - (v.x_cell - (long)A * K) || v.cells == 0,
                 "%s: level %d logits image stride %ld", what, l, v.x_img);
    JTSM_REQUIRE(v.d_img >= (long)v.cells * v.d_cell - (v.d_cell - 4L * A) || v.cells == 0,
                 "%s: level %d deltas image stride %ld", what, l, v.d_img);
    v.upc = 0;
    v.unit0 = 0;
  }
  JTSM_REQUIRE(rows == R, "%s: the levels hold %ld anchors, R=%ld", what, rows, R);
  return JTSM_OK;
}

// 16-byte accesses along a cell: four floats never straddle a row, every cell and image starts on a multiple of four
bool vec_ok(const Table& T, int K, bool on_deltas) {
  if (K % 4) return false;
  for (int l = 0; l < T.L; ++l) {
    const Level& v = T.lv[l];
    if (!on_deltas && ((v.x_cell % 4) || (v.x_img % 4) || ((uintptr_t)v.x % 16))) return false;
    if (on_deltas && ((v.d_cell % 4) || (v.d_img % 4) || ((uintptr_t)v.d % 16))) return false;
  }
  return true;
}

void plan_units(Table& T, int N, const int* upc) {
  long u = 0;
  for (int l = 0; l < T.L; ++l) {
    T.lv[l].upc = upc[l];
    T.lv[l].unit0 = u;
    u += (long)N * T.lv[l].cells * upc[l];
  }
  T.units = u;
}

int grid_for(long units, int per_thread) {
  const long g = (units + (long)kThreads * per_thread - 1) / ((long)kThreads * per_thread);
  return (int)(g < 1 ? 1 : g > kMaxGrid ? kMaxGrid : g);
}

// unit u -> level, image, cell, unit within the cell
__device__ __forceinline__ int locate(const Table& T, long u, int& n, int& cell, int& j) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < kMaxLevels; ++i)
    if (i < T.L && u >= T.lv[i].unit0) l = i;
  const Level& v = T.lv[l];
  const long rem = u - v.unit0, per_img = (long)v.cells * v.upc;
  n = (int)(rem / per_img);
  const unsigned r2 = (unsigned)(rem - (long)n * per_img);
  cell = (int)(r2 / (unsigned)v.upc);
  j = (int)(r2 - (unsigned)cell * (unsigned)v.upc);
  return l;
}

template <int V>
__device__ __forceinline__ void load_v(const float* __restrict__ p, float (&x)[V]) {
  if (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    x[0] = q.x; x[V > 1 ? 1 : 0] = q.y; x[V > 2 ? 2 : 0] = q.z; x[V > 3 ? 3 : 0] = q.w;
  } else {
    x[0] = p[0];
  }
}
template <int V>
__device__ __forceinline__ void store_v(float* __restrict__ p, const float (&x)[V]) {
  if (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(x[0], x[V > 1 ? 1 : 0], x[V > 2 ? 2 : 0], x[V > 3 ? 3 : 0]);
  } else {
    p[0] = x[0];
  }
}

// ---- a. labels -----------------------------------------------------------------------------------------------------
struct Intervals {
  float thr[kMaxThresholds];
  int lab[kMaxThresholds + 1];
  int nt;
};

// pass 1: gmax[g] <- the largest IoU of gt g with any anchor, as the bits of a non-negative float (a max: order-free)
__global__ __launch_bounds__(kThreads) void gt_max_kernel(const float* __restrict__ anchors, int R,
                                                          const float* __restrict__ gt,
                                                          const int* __restrict__ offsets,
                                                          unsigned* __restrict__ gmax) {
  __shared__ float4 sb[kChunk];
  const int n = blockIdx.y, r = blockIdx.x * kThreads + threadIdx.x;
  const int g0 = offsets[n], g1 = offsets[n + 1];
  const bool live = r < R;
  const float4 a = live ? box_at(anchors, r) : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int base = g0; base < g1; base += kChunk) {
    const int cnt = min(kChunk, g1 - base);
    __syncthreads();
    if ((int)threadIdx.x < cnt) sb[threadIdx.x] = box_at(gt, base + threadIdx.x);
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const float v = live ? box_iou(sb[j], a) : 0.f;
      if (__any(v > 0.f)) {                                   // (a zero maximum is what the buffer starts from)
        const float m = wave_max(v);
        if ((threadIdx.x & 63) == 0) atomicMax(&gmax[base + j], __float_as_uint(m));
      }
    }
  }
}

// pass 2: Matcher.__call__ + set_low_quality_matches_ + label_anchors' class look-up; the IoUs are formed again
__global__ __launch_bounds__(kThreads) void label_kernel(const float* __restrict__ anchors, int R,
                                                         const float* __restrict__ gt, const int* __restrict__ offsets,
                                                         const int64_t* __restrict__ classes,
                                                         const unsigned* __restrict__ gmax, Intervals iv, int K,
                                                         int* __restrict__ labels, int* __restrict__ matched,
                                                         int* __restrict__ num_pos) {
  __shared__ float4 sb[kChunk];
  __shared__ float sm[kChunk];
  const int n = blockIdx.y, r = blockIdx.x * kThreads + threadIdx.x;
  const int g0 = offsets[n], g1 = offsets[n + 1];
  const bool live = r < R;
  const float4 a = live ? box_at(anchors, r) : make_float4(0.f, 0.f, 0.f, 0.f);
  float bv = -1.f;
  int bi = 0;
  bool low = false;
  for (int base = g0; base < g1; base += kChunk) {
    const int cnt = min(kChunk, g1 - base);
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
      sb[threadIdx.x] = box_at(gt, base + threadIdx.x);
      sm[threadIdx.x] = __uint_as_float(gmax[base + threadIdx.x]);
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const float v = box_iou(sb[j], a);
      if (v > bv) { bv = v; bi = base + j - g0; }             // j grows: a tie keeps the lowest gt index
      low = low || v == sm[j];
    }
  }
  int out = K, pos = 0;
  if (live) {
    if (g1 > g0) {
      int l = 1;
      float lo = -INFINITY;
      for (int i = 0; i <= iv.nt; ++i) {
        const float hi = i < iv.nt ? iv.thr[i] : INFINITY;
        if (bv >= lo && bv < hi) l = iv.lab[i];
        lo = hi;
      }
      if (low) l = 1;
      out = l == 1 ? (int)classes[g0 + bi] : (l == 0 ? K : -1);
    }
    pos = out >= 0 && out != K;
    labels[(long)n * R + r] = out;
    matched[(long)n * R + r] = bi;
  }
  const int c = wave_sum(pos);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(num_pos, c);
}

// ---- b. losses -----------------------------------------------------------------------------------------------------
struct LossParams {
  float alpha, gamma, beta;
  int gmode;                // 0: gamma == 0, 1: gamma == 2, 2: powf
  float wx, wy, ww, wh;
};

// sigmoid_focal_loss for one element: the value, and its derivative by x when G.  One exp(-|x|) serves p and ce.
template <bool G>
__device__ __forceinline__ float focal(float x, bool t, const LossParams& P, float& grad) {
  const float e = expf(-fabsf(x));
  const float s = 1.f / (1.f + e);
  const float p = x >= 0.f ? s : e * s, omp = x >= 0.f ? e * s : s;          // sigmoid(x), 1 - sigmoid(x)
  const float ce = fmaxf(x, 0.f) - (t ? x : 0.f) + log1pf(e);
  const float q = t ? omp : p;                                                // 1 - p_t
  const float mod = P.gmode == 1 ? q * q : (P.gmode == 0 ? 1.f : powf(q, P.gamma));
  const float at = P.alpha >= 0.f ? (t ? P.alpha : 1.f - P.alpha) : 1.f;
  if (G) {
    const float dmod = P.gmode == 1 ? 2.f * q : (P.gmode == 0 ? 0.f : P.gamma * powf(q, P.gamma - 1.f));
    const float dq = t ? -(p * omp) : p * omp;
    grad = at * ((p - (t ? 1.f : 0.f)) * mod + ce * dmod * dq);
  }
  return at * mod * ce;
}

template <int V>
__global__ __launch_bounds__(kThreads) void focal_forward_kernel(Table T, int A, int K, long R,
                                                                 const int* __restrict__ labels, LossParams P,
                                                                 double* __restrict__ partial) {
  __shared__ double part[kWaves];
  double acc = 0.0;
  for (long u = (long)blockIdx.x * kThreads + threadIdx.x; u < T.units; u += (long)gridDim.x * kThreads) {
    int n, cell, j;
    const Level& lv = T.lv[locate(T, u, n, cell, j)];
    const int e = j * V, a = e / K, k = e - a * K;
    const int lab = labels[(long)n * R + lv.off + cell * A + a];
    if (lab < 0) continue;
    float x[V], g;
    load_v<V>(lv.x + (long)n * lv.x_img + (long)cell * lv.x_cell + e, x);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) s += focal<false>(x[i], k + i == lab, P, g);
    acc += (double)s;
  }
  acc = wg_reduce<kWaves>(acc, Add(), part);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// Box2BoxTransform.get_deltas(anchor, gt) in its operation order
__device__ __forceinline__ void target_deltas(const float4 s, const float4 t, const LossParams& P, float (&d)[4]) {
  const float sw = s.z - s.x, sh = s.w - s.y;
  const float scx = s.x + 0.5f * sw, scy = s.y + 0.5f * sh;
  const float tw = t.z - t.x, th = t.w - t.y;
  const float tcx = t.x + 0.5f * tw, tcy = t.y + 0.5f * th;
  d[0] = P.wx * (tcx - scx) / sw;
  d[1] = P.wy * (tcy - scy) / sh;
  d[2] = P.ww * logf(tw / sw);
  d[3] = P.wh * logf(th / sh);
}

__device__ __forceinline__ float smooth_l1(float d, float beta, float& grad) {
  const float ad = fabsf(d), sign = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  if (beta < 1e-5f) { grad = sign; return ad; }
  if (ad < beta) { grad = d / beta; return 0.5f * d * d / beta; }
  grad = sign;
  return ad - 0.5f * beta;
}

// one thread per (image, anchor)
__global__ __launch_bounds__(kThreads) void box_forward_kernel(Table T, int N, int A, int K, long R,
                                                               const int* __restrict__ labels,
                                                               const int* __restrict__ matched,
                                                               const float* __restrict__ anchors,
                                                               const float* __restrict__ gt,
                                                               const int* __restrict__ offsets, LossParams P,
                                                               double* __restrict__ partial) {
  __shared__ double part[kWaves];
  double acc = 0.0;
  for (long u = (long)blockIdx.x * kThreads + threadIdx.x; u < T.units; u += (long)gridDim.x * kThreads) {
    int n, cell, a;
    const Level& lv = T.lv[locate(T, u, n, cell, a)];
    const long r = lv.off + (long)cell * A + a;
    const int lab = labels[(long)n * R + r];
    if (lab < 0 || lab == K) continue;
    float want[4], g;
    target_deltas(box_at(anchors, r), box_at(gt, offsets[n] + matched[(long)n * R + r]), P, want);
    const float* __restrict__ d = lv.d + (long)n * lv.d_img + (long)cell * lv.d_cell + a * 4;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += smooth_l1(d[i] - want[i], P.beta, g);
    acc += (double)s;
  }
  acc = wg_reduce<kWaves>(acc, Add(), part);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// saved for the backward: the fp32 normaliser the forward divided by
struct LossSaved {
  float norm;
};

__global__ __launch_bounds__(kThreads) void loss_final_kernel(const double* __restrict__ pc, int nc,
                                                              const double* __restrict__ pb, int nb,
                                                              const int* __restrict__ num_pos,
                                                              double* __restrict__ normalizer, double momentum,
                                                              int training, float* __restrict__ loss_cls,
                                                              float* __restrict__ loss_box,
                                                              LossSaved* __restrict__ saved) {
  __shared__ double part[kWaves];
  double c = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nc; i += kThreads) c += pc[i];
  for (int i = threadIdx.x; i < nb; i += kThreads) b += pb[i];
  c = wg_reduce<kWaves>(c, Add(), part);
  b = wg_reduce<kWaves>(b, Add(), part);
  if (threadIdx.x == 0) {
    double nrm = *normalizer;
    if (training) {
      const int np = *num_pos;
      nrm = momentum * nrm + (1.0 - momentum) * (double)(np > 1 ? np : 1);
      *normalizer = nrm;
    }
    const float f = (float)nrm;
    saved->norm = f;
    *loss_cls = (float)c / f;
    *loss_box = (float)b / f;
  }
}

// every float of every cell of the gradient map is written: padding and ignored anchors get zeros
template <int V>
__global__ __launch_bounds__(kThreads) void focal_backward_kernel(Table T, Table Gd, int A, int K, long R,
                                                                  const int* __restrict__ labels, LossParams P,
                                                                  const float* __restrict__ up,
                                                                  const LossSaved* __restrict__ saved) {
  const float scale = *up / saved->norm;
  for (long u = (long)blockIdx.x * kThreads + threadIdx.x; u < Gd.units; u += (long)gridDim.x * kThreads) {
    int n, cell, j;
    const int l = locate(Gd, u, n, cell, j);
    const Level& lv = T.lv[l];
    const Level& gv = Gd.lv[l];
    const int e = j * V;
    float g[V];
#pragma unroll
    for (int i = 0; i < V; ++i) g[i] = 0.f;
    if (e < A * K) {
      const int a = e / K, k = e - a * K;
      const int lab = labels[(long)n * R + lv.off + cell * A + a];
      if (lab >= 0) {
        float x[V];
        load_v<V>(lv.x + (long)n * lv.x_img + (long)cell * lv.x_cell + e, x);
#pragma unroll
        for (int i = 0; i < V; ++i) {
          float d;
          focal<true>(x[i], k + i == lab, P, d);
          g[i] = d * scale;
        }
      }
    }
    store_v<V>(const_cast<float*>(gv.x) + (long)n * gv.x_img + (long)cell * gv.x_cell + e, g);
  }
}

// one thread per float of a cell of the deltas' gradient map
__global__ __launch_bounds__(kThreads) void box_backward_kernel(Table T, Table Gd, int A, int K, long R,
                                                                const int* __restrict__ labels,
                                                                const int* __restrict__ matched,
                                                                const float* __restrict__ anchors,
                                                                const float* __restrict__ gt,
                                                                const int* __restrict__ offsets, LossParams P,
                                                                const float* __restrict__ up,
                                                                const LossSaved* __restrict__ saved) {
  const float scale = *up / saved->norm;
  for (long u = (long)blockIdx.x * kThreads + threadIdx.x; u < Gd.units; u += (long)gridDim.x * kThreads) {
    int n, cell, e;
    const int l = locate(Gd, u, n, cell, e);
    const Level& lv = T.lv[l];
    const Level& gv = Gd.lv[l];
    float g = 0.f;
    if (e < 4 * A) {
      const int a = e >> 2, i = e & 3;
      const long r = lv.off + (long)cell * A + a;
      const int lab = labels[(long)n * R + r];
      if (lab >= 0 && lab != K) {
        float want[4];
        target_deltas(box_at(anchors, r), box_at(gt, offsets[n] + matched[(long)n * R + r]), P, want);
        const float d = lv.d[(long)n * lv.d_img + (long)cell * lv.d_cell + e];
        smooth_l1(d - want[i], P.beta, g);
        g *= scale;
      }
    }
    const_cast<float*>(gv.d)[(long)n * gv.d_img + (long)cell * gv.d_cell + e] = g;
  }
}

struct LossLayout {
  double* pc;
  double* pb;
  LossSaved* saved;
};
LossLayout carve_loss(Arena& A) {
  LossLayout o;
  o.pc = A.take<double>(kMaxGrid);
  o.pb = A.take<double>(kMaxGrid);
  o.saved = A.take<LossSaved>(1);
  return o;
}

int fill_params(LossParams& P, float alpha, float gamma, float beta, const float* w, const char* what) {
  JTSM_REQUIRE(w, "%s: null weights", what);
  JTSM_REQUIRE(gamma >= 0.f && beta >= 0.f, "%s: gamma=%g beta=%g", what, gamma, beta);
  P.alpha = alpha;
  P.gamma = gamma;
  P.beta = beta;
  P.gmode = gamma == 0.f ? 0 : (gamma == 2.f ? 1 : 2);
  P.wx = w[0]; P.wy = w[1]; P.ww = w[2]; P.wh = w[3];
  return JTSM_OK;
}

// ---- c. candidates -------------------------------------------------------------------------------------------------
// An element that passes the threshold has the key (score bits << 32) | (2^32 - 1 - flat index): scores are positive
// floats, so a larger key is an earlier place — score descending, then flat index ascending — and no two keys of a
// segment (image, level) are equal.  The topk-th largest key is found by a radix select, one 16-bit digit per pass
// from the top: a histogram of the digit over the elements that match the digits chosen so far, then the bin where
// the count from the top reaches what is still wanted.  A pass after which the whole bin is wanted (no excess ties)
// ends the search; so do fewer than topk passing elements.  The workspace is the histograms and topk keys per
// segment, whatever passes.
struct SegState {
  u64 prefix;      // digits chosen so far, in key position
  u64 cut;         // keys >= cut are the selection (valid once done)
  int remaining;   // still wanted among the elements matching prefix
  int done;
  int count;       // survivors compacted
  int pad;
};

__device__ __forceinline__ bool candidate_key(float x, float thresh, unsigned flat, u64& key) {
  const float s = 1.f / (1.f + expf(-x));
  if (!(s > thresh)) return false;                      // (a NaN never passes)
  key = ((u64)__float_as_uint(s) << 32) | (u64)(0xffffffffu - flat);
  return true;
}

template <int V>
__global__ __launch_bounds__(kThreads) void cand_hist_kernel(Table T, int A, int K, float thresh, int pass,
                                                             const SegState* __restrict__ st, int segs,
                                                             unsigned* __restrict__ hist) {
  const int lane = threadIdx.x & 63;
  if (pass > 0) {                                             // (uniform) every segment has its cut: nothing to count
    bool all = true;
    for (int i = 0; i < segs; ++i) all = all && st[i].done != 0;
    if (all) return;
  }
  for (long u = (long)blockIdx.x * kThreads + threadIdx.x; u < T.units; u += (long)gridDim.x * kThreads) {
    int n, cell, j;
    const int l = locate(T, u, n, cell, j);
    const Level& lv = T.lv[l];
    const int seg = n * T.L + l;
    const SegState S = st[seg];
    if (S.done) continue;
    float x[V];
    load_v<V>(lv.x + (long)n * lv.x_img + (long)cell * lv.x_cell + j * V, x);
    const unsigned flat0 = (unsigned)cell * (unsigned)(A * K) + (unsigned)(j * V);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      u64 key = 0;
      bool in = candidate_key(x[i], thresh, flat0 + i, key);
      if (in && pass > 0) in = (key >> (64 - 16 * pass)) == (S.prefix >> (64 - 16 * pass));
      const unsigned bin = (unsigned)seg * kBins + (unsigned)((key >> (48 - 16 * pass)) & 0xffffu);
      // Scores crowd into few bins (an untrained head: every score near the prior; saturated logits: one bin), and
      // 64 atomics per wavefront on one address serialise.  Up to four rounds in which the first waiting lane's bin is
      // added once for all lanes that share it; what is left after them adds for itself.
      u64 m = __ballot(in);
      for (int round = 0; m && round < 4; ++round) {
        const int leader = __ffsll((long long)m) - 1;
        const unsigned lbin = __shfl(bin, leader);
        const bool same = in && bin == lbin;
        const u64 sm = __ballot(same);
        if (lane == leader) atomicAdd(&hist[lbin], (unsigned)__popcll(sm));
        in = in && !same;
        m = __ballot(in);
      }
      if (in) atomicAdd(&hist[bin], 1u);
    }
  }
}

// one workgroup per segment: thread t owns bins 65535 - 64 t down to 65535 - 64 t - 63
__global__ __launch_bounds__(kSelectThreads) void cand_select_kernel(SegState* __restrict__ st,
                                                                     unsigned* __restrict__ hist, int pass) {
  __shared__ unsigned sums[kSelectThreads];
  __shared__ int owner;
  __shared__ unsigned before;
  const int seg = blockIdx.x, t = threadIdx.x;
  if (st[seg].done) return;                                   // (uniform; its bins were never touched)
  unsigned* __restrict__ h = hist + (long)seg * kBins;
  const int per = kBins / kSelectThreads, top = kBins - 1 - t * per;
  const int remaining = st[seg].remaining;
  unsigned s = 0;
  for (int b = 0; b < per; ++b) s += h[top - b];
  sums[t] = s;
  __syncthreads();
  if (t == 0) {
    unsigned cum = 0;
    int own = -1;
    for (int i = 0; i < kSelectThreads; ++i) {
      if (cum + sums[i] >= (unsigned)remaining) { own = i; break; }
      cum += sums[i];
    }
    owner = own;
    before = cum;
    if (own < 0) {                    // fewer than wanted: everything that matches the prefix is taken
      st[seg].cut = st[seg].prefix;
      st[seg].done = 1;
    }
  }
  __syncthreads();
  if (t == owner) {
    unsigned cum = before;
    int digit = top - per + 1;
    unsigned in_bin = 0;
    for (int b = 0; b < per; ++b) {
      const unsigned c = h[top - b];
      if (cum + c >= (unsigned)remaining) { digit = top - b; in_bin = c; break; }
      cum += c;
    }
    const u64 prefix = st[seg].prefix | ((u64)digit << (48 - 16 * pass));
    const int left = remaining - (int)cum;
    st[seg].prefix = prefix;
    st[seg].remaining = left;
    if (in_bin == (unsigned)left || pass == 3) {
      st[seg].cut = prefix;
      st[seg].done = 1;
    }
  }
  __syncthreads();
  for (int b = 0; b < per; ++b) h[top - b] = 0;               // for the next pass
}

__global__ void cand_init_kernel(SegState* __restrict__ st, int segs, int topk) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= segs) return;
  SegState S;
  S.prefix = 0; S.cut = 0; S.remaining = topk; S.done = topk <= 0; S.count = 0; S.pad = 0;
  if (topk <= 0) S.cut = ~(u64)0;
  st[i] = S;
}

template <int V>
__global__ __launch_bounds__(kThreads) void cand_compact_kernel(Table T, int A, int K, float thresh, int topk,
                                                                SegState* __restrict__ st, u64* __restrict__ surv) {
  for (long u = (long)blockIdx.x * kThreads + threadIdx.x; u < T.units; u += (long)gridDim.x * kThreads) {
    int n, cell, j;
    const int l = locate(T, u, n, cell, j);
    const Level& lv = T.lv[l];
    const int seg = n * T.L + l;
    const u64 cut = st[seg].cut;
    float x[V];
    load_v<V>(lv.x + (long)n * lv.x_img + (long)cell * lv.x_cell + j * V, x);
    const unsigned flat0 = (unsigned)cell * (unsigned)(A * K) + (unsigned)(j * V);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      u64 key;
      if (candidate_key(x[i], thresh, flat0 + i, key) && key >= cut) {
        const int slot = atomicAdd(&st[seg].count, 1);
        if (slot < topk) surv[(long)seg * topk + slot] = key;
      }
    }
  }
}

// Box2BoxTransform(weights, scale_clamp).apply_deltas for one box, in decode_box's order (box_math.h)
__device__ __forceinline__ void decode_weighted(const float4 p, const float* __restrict__ d, const LossParams& P,
                                                float clamp, float* out) {
  const float w = p.z - p.x, h = p.w - p.y;
  const float cx = p.x + 0.5f * w, cy = p.y + 0.5f * h;
  const float dx = d[0] / P.wx, dy = d[1] / P.wy;
  const float dw = fminf(d[2] / P.ww, clamp), dh = fminf(d[3] / P.wh, clamp);
  const float pcx = dx * w + cx, pcy = dy * h + cy;
  const float pw = expf(dw) * w, ph = expf(dh) * h;
  out[0] = pcx - 0.5f * pw;
  out[1] = pcy - 0.5f * ph;
  out[2] = pcx + 0.5f * pw;
  out[3] = pcy + 0.5f * ph;
}

// one workgroup per segment: a survivor's place is the number of survivors with a larger key
__global__ __launch_bounds__(kThreads) void cand_emit_kernel(Table T, int A, int K, int topk,
                                                             const SegState* __restrict__ st,
                                                             const u64* __restrict__ surv,
                                                             const float* __restrict__ anchors, LossParams P,
                                                             float clamp, float* __restrict__ boxes,
                                                             float* __restrict__ scores, int64_t* __restrict__ classes,
                                                             int* __restrict__ rows, int* __restrict__ counts) {
  __shared__ u64 tile[kThreads];
  const int seg = blockIdx.x, n = seg / T.L, l = seg - n * T.L;
  const Level& lv = T.lv[l];
  const int cnt = min(st[seg].count, topk);
  const u64* __restrict__ keys = surv + (long)seg * topk;
  if (threadIdx.x == 0) counts[seg] = cnt;
  for (int base = 0; base < topk; base += kThreads) {        // (uniform trip count: the barriers below)
    const int i = base + threadIdx.x;
    const u64 mine = i < cnt ? keys[i] : 0;
    int rank = 0;
    for (int tb = 0; tb < cnt; tb += kThreads) {
      __syncthreads();
      tile[threadIdx.x] = tb + (int)threadIdx.x < cnt ? keys[tb + threadIdx.x] : 0;
      __syncthreads();
      const int m = min(kThreads, cnt - tb);
      for (int q = 0; q < m; ++q) rank += tile[q] > mine;
    }
    if (i < cnt) {
      const long o = (long)seg * topk + rank;
      const unsigned flat = 0xffffffffu - (unsigned)(mine & 0xffffffffull);
      const unsigned row = flat / (unsigned)K, cls = flat - row * (unsigned)K;
      const unsigned cell = row / (unsigned)A, a = row - cell * (unsigned)A;
      decode_weighted(box_at(anchors, lv.off + (long)row), lv.d + (long)n * lv.d_img + (long)cell * lv.d_cell + a * 4,
                      P, clamp, boxes + 4 * o);
      scores[o] = __uint_as_float((unsigned)(mine >> 32));
      classes[o] = (int64_t)cls;
      if (rows) rows[o] = (int)row;
    } else if (i < topk) {
      const long o = (long)seg * topk + i;                    // (places cnt .. topk - 1: no survivor ranks there)
      boxes[4 * o] = boxes[4 * o + 1] = boxes[4 * o + 2] = boxes[4 * o + 3] = 0.f;
      scores[o] = 0.f;
      classes[o] = -1;
      if (rows) rows[o] = -1;
    }
  }
}

struct CandLayout {
  SegState* st;
  unsigned* hist;
  u64* surv;
  size_t clear_end;
};
CandLayout carve_candidates(Arena& A, int N, int L, int topk) {
  CandLayout o;
  const size_t segs = (size_t)(N > 0 ? N : 0) * (size_t)(L > 0 ? L : 0);
  o.st = A.take<SegState>(segs);
  o.hist = A.take<unsigned>(segs * kBins);
  o.clear_end = A.mark();
  o.surv = A.take<u64>(segs * (size_t)(topk > 0 ? topk : 0));
  return o;
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" {

size_t jtsm_retinanet_label_workspace_bytes(int total_gt) {
  Arena A{nullptr};
  A.take<unsigned>((size_t)(total_gt > 0 ? total_gt : 0));
  return A.off + 256;
}

int jtsm_retinanet_label_anchors_f32(const float* anchors, int R, const float* gt_boxes, const int32_t* gt_offsets,
                                     const int64_t* gt_classes, int N, int total_gt, const float* thresholds,
                                     const int32_t* interval_labels, int num_thresholds, int num_classes,
                                     int32_t* labels, int32_t* matched, int32_t* num_pos, void* workspace,
                                     void* stream) {
  JTSM_REQUIRE(R >= 0 && N >= 0 && N < 65536 && total_gt >= 0 && num_classes >= 1,
               "retinanet_label_anchors: R=%d N=%d G=%d K=%d", R, N, total_gt, num_classes);
  JTSM_REQUIRE(num_thresholds >= 0 && num_thresholds <= kMaxThresholds && thresholds && interval_labels,
               "retinanet_label_anchors: %d thresholds (0..%d)", num_thresholds, kMaxThresholds);
  JTSM_REQUIRE(num_pos, "retinanet_label_anchors: null pointer");
  Intervals iv;
  iv.nt = num_thresholds;
  for (int i = 0; i < num_thresholds; ++i) {
    JTSM_REQUIRE(i == 0 || thresholds[i] >= thresholds[i - 1], "retinanet_label_anchors: thresholds must ascend");
    iv.thr[i] = thresholds[i];
  }
  for (int i = 0; i <= num_thresholds; ++i) {
    JTSM_REQUIRE(interval_labels[i] >= -1 && interval_labels[i] <= 1, "retinanet_label_anchors: label %d",
                 interval_labels[i]);
    iv.lab[i] = interval_labels[i];
  }
  hipStream_t s = as_stream(stream);
  JTSM_CHECK_HIP(hipMemsetAsync(num_pos, 0, sizeof(int32_t), s));
  if (R == 0 || N == 0) return JTSM_OK;
  JTSM_REQUIRE(anchors && gt_offsets && labels && matched && workspace, "retinanet_label_anchors: null pointer");
  JTSM_REQUIRE(total_gt == 0 || (gt_boxes && gt_classes), "retinanet_label_anchors: null gt");
  unsigned* gmax = (unsigned*)workspace;
  const dim3 grid(ceil_div(R, kThreads), N);
  if (total_gt) {
    JTSM_CHECK_HIP(hipMemsetAsync(gmax, 0, (size_t)total_gt * sizeof(unsigned), s));
    hipLaunchKernelGGL(gt_max_kernel, grid, dim3(kThreads), 0, s, anchors, R, gt_boxes, gt_offsets, gmax);
    JTSM_CHECK_LAUNCH("retinanet_label_anchors gt max");
  }
  hipLaunchKernelGGL(label_kernel, grid, dim3(kThreads), 0, s, anchors, R, gt_boxes, gt_offsets, gt_classes, gmax, iv,
                     num_classes, labels, matched, num_pos);
  JTSM_CHECK_LAUNCH("retinanet_label_anchors labels");
  return JTSM_OK;
}

size_t jtsm_retinanet_loss_workspace_bytes(void) {
  Arena A{nullptr};
  carve_loss(A);
  return A.off;
}

int jtsm_retinanet_loss_forward_f32(const float* const* logits, const float* const* deltas, const int64_t* geom,
                                    int L, int N, int A, int K, int R, const int32_t* labels, const int32_t* matched,
                                    const float* anchors, const float* gt_boxes, const int32_t* gt_offsets,
                                    float alpha, float gamma, float beta, const float* weights,
                                    const int32_t* num_pos, double* normalizer, double momentum, int training,
                                    float* loss_cls, float* loss_box_reg, void* workspace, void* stream) {
  Table T;
  if (int rc = fill_table(T, logits, deltas, geom, L, N, A, K, R, "retinanet_loss")) return rc;
  LossParams P;
  if (int rc = fill_params(P, alpha, gamma, beta, weights, "retinanet_loss")) return rc;
  JTSM_REQUIRE(normalizer && loss_cls && loss_box_reg && workspace && (num_pos || !training),
               "retinanet_loss: null pointer");
  Arena Ar{(char*)workspace};
  const LossLayout W = carve_loss(Ar);
  hipStream_t s = as_stream(stream);
  int gc = 0, gb = 0;
  if ((long)N * R > 0) {
    JTSM_REQUIRE(logits && deltas && labels && matched && anchors && gt_offsets, "retinanet_loss: null pointer");
    for (int l = 0; l < L; ++l)
      JTSM_REQUIRE((logits[l] && deltas[l]) || T.lv[l].cells == 0, "retinanet_loss: null level %d", l);
    const bool vec = vec_ok(T, K, false);
    int upc[kMaxLevels];
    for (int l = 0; l < L; ++l) upc[l] = vec ? A * K / 4 : A * K;
    plan_units(T, N, upc);
    gc = grid_for(T.units, vec ? 2 : 8);
    if (vec)
      hipLaunchKernelGGL(focal_forward_kernel<4>, dim3(gc), dim3(kThreads), 0, s, T, A, K, (long)R, labels, P, W.pc);
    else
      hipLaunchKernelGGL(focal_forward_kernel<1>, dim3(gc), dim3(kThreads), 0, s, T, A, K, (long)R, labels, P, W.pc);
    JTSM_CHECK_LAUNCH("retinanet_loss focal");
    for (int l = 0; l < L; ++l) upc[l] = A;
    plan_units(T, N, upc);
    gb = grid_for(T.units, 1);
    hipLaunchKernelGGL(box_forward_kernel, dim3(gb), dim3(kThreads), 0, s, T, N, A, K, (long)R, labels, matched,
                       anchors, gt_boxes, gt_offsets, P, W.pb);
    JTSM_CHECK_LAUNCH("retinanet_loss box");
  }
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(kThreads), 0, s, W.pc, gc, W.pb, gb, num_pos, normalizer,
                     momentum, training, loss_cls, loss_box_reg, W.saved);
  JTSM_CHECK_LAUNCH("retinanet_loss final");
  return JTSM_OK;
}

int jtsm_retinanet_loss_backward_f32(const float* const* logits, const float* const* deltas, const int64_t* geom,
                                     int L, int N, int A, int K, int R, const int32_t* labels, const int32_t* matched,
                                     const float* anchors, const float* gt_boxes, const int32_t* gt_offsets,
                                     float alpha, float gamma, float beta, const float* weights,
                                     const float* grad_cls, const float* grad_box_reg, const void* workspace,
                                     float* const* grad_logits, float* const* grad_deltas, const int64_t* grad_geom,
                                     void* stream) {
  Table T, Gd;
  if (int rc = fill_table(T, logits, deltas, geom, L, N, A, K, R, "retinanet_loss_backward")) return rc;
  if (int rc = fill_table(Gd, grad_logits, grad_deltas, grad_geom, L, N, A, K, R, "retinanet_loss_backward")) return rc;
  LossParams P;
  if (int rc = fill_params(P, alpha, gamma, beta, weights, "retinanet_loss_backward")) return rc;
  if ((long)N * R == 0) return JTSM_OK;
  JTSM_REQUIRE(logits && deltas && grad_logits && grad_deltas && labels && matched && anchors && gt_offsets &&
               grad_cls && grad_box_reg && workspace, "retinanet_loss_backward: null pointer");
  for (int l = 0; l < L; ++l)
    JTSM_REQUIRE((logits[l] && deltas[l] && grad_logits[l] && grad_deltas[l]) || T.lv[l].cells == 0,
                 "retinanet_loss_backward: null level %d", l);
  Arena Ar{(char*)const_cast<void*>(workspace)};
  const LossLayout W = carve_loss(Ar);
  hipStream_t s = as_stream(stream);
  // the gradient maps' last cell is written whole: the image stride must hold it
  for (int l = 0; l < L; ++l) {
    const Level& v = Gd.lv[l];
    JTSM_REQUIRE(v.cells == 0 || (v.x_img >= (long)v.cells * v.x_cell && v.d_img >= (long)v.cells * v.d_cell),
                 "retinanet_loss_backward: level %d gradient maps must hold whole cells", l);
  }
  const bool vec = vec_ok(T, K, false) && vec_ok(Gd, K, false);
  int upc[kMaxLevels];
  for (int l = 0; l < L; ++l) upc[l] = vec ? Gd.lv[l].x_cell / 4 : Gd.lv[l].x_cell;
  plan_units(Gd, N, upc);
  const int gc = grid_for(Gd.units, vec ? 2 : 8);
  if (vec)
    hipLaunchKernelGGL(focal_backward_kernel<4>, dim3(gc), dim3(kThreads), 0, s, T, Gd, A, K, (long)R, labels, P,
                       grad_cls, W.saved);
  else
    hipLaunchKernelGGL(focal_backward_kernel<1>, dim3(gc), dim3(kThreads), 0, s, T, Gd, A, K, (long)R, labels, P,
                       grad_cls, W.saved);
  JTSM_CHECK_LAUNCH("retinanet_loss_backward focal");
  for (int l = 0; l < L; ++l) upc[l] = Gd.lv[l].d_cell;
  plan_units(Gd, N, upc);
  hipLaunchKernelGGL(box_backward_kernel, dim3(grid_for(Gd.units, 4)), dim3(kThreads), 0, s, T, Gd, A, K, (long)R,
                     labels, matched, anchors, gt_boxes, gt_offsets, P, grad_box_reg, W.saved);
  JTSM_CHECK_LAUNCH("retinanet_loss_backward box");
  return JTSM_OK;
}

size_t jtsm_retinanet_candidates_workspace_bytes(int N, int L, int topk) {
  Arena A{nullptr};
  carve_candidates(A, N, L, topk);
  return A.off;
}

int jtsm_retinanet_candidates_f32(const float* const* logits, const float* const* deltas, const int64_t* geom, int L,
                                  int N, int A, int K, int R, const float* anchors, const float* weights,
                                  float scale_clamp, float score_thresh, int topk, float* boxes, float* scores,
                                  int64_t* classes, int32_t* rows, int32_t* counts, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  Table T;
  if (int rc = fill_table(T, logits, deltas, geom, L, N, A, K, R, "retinanet_candidates")) return rc;
  LossParams P;
  if (int rc = fill_params(P, -1.f, 0.f, 0.f, weights, "retinanet_candidates")) return rc;
  JTSM_REQUIRE(topk >= 0 && (long)N * L * topk < (1L << 31), "retinanet_candidates: topk=%d", topk);
  if (N == 0) return JTSM_OK;
  JTSM_REQUIRE(logits && deltas && anchors && boxes && scores && classes && counts && workspace,
               "retinanet_candidates: null pointer");
  for (int l = 0; l < L; ++l)
    JTSM_REQUIRE((logits[l] && deltas[l]) || T.lv[l].cells == 0, "retinanet_candidates: null level %d", l);
  Arena Ar{(char*)workspace};
  const CandLayout W = carve_candidates(Ar, N, L, topk);
  JTSM_REQUIRE(workspace_bytes >= Ar.off, "retinanet_candidates: workspace %zu < %zu", workspace_bytes, Ar.off);
  hipStream_t s = as_stream(stream);
  const int segs = N * L;
  JTSM_CHECK_HIP(hipMemsetAsync(workspace, 0, W.clear_end, s));
  hipLaunchKernelGGL(cand_init_kernel, dim3(ceil_div(segs, 64)), dim3(64), 0, s, W.st, segs, topk);
  JTSM_CHECK_LAUNCH("retinanet_candidates init");
  const bool vec = vec_ok(T, K, false);
  int upc[kMaxLevels];
  for (int l = 0; l < L; ++l) upc[l] = vec ? A * K / 4 : A * K;
  plan_units(T, N, upc);
  const int grid = grid_for(T.units, vec ? 2 : 8);
  if (T.units > 0 && topk > 0) {
    for (int pass = 0; pass < 4; ++pass) {
      if (vec)
        hipLaunchKernelGGL(cand_hist_kernel<4>, dim3(grid), dim3(kThreads), 0, s, T, A, K, score_thresh, pass, W.st,
                           segs, W.hist);
      else
        hipLaunchKernelGGL(cand_hist_kernel<1>, dim3(grid), dim3(kThreads), 0, s, T, A, K, score_thresh, pass, W.st,
                           segs, W.hist);
      JTSM_CHECK_LAUNCH("retinanet_candidates histogram");
      hipLaunchKernelGGL(cand_select_kernel, dim3(segs), dim3(kSelectThreads), 0, s, W.st, W.hist, pass);
      JTSM_CHECK_LAUNCH("retinanet_candidates select");
    }
    if (vec)
      hipLaunchKernelGGL(cand_compact_kernel<4>, dim3(grid), dim3(kThreads), 0, s, T, A, K, score_thresh, topk, W.st,
                         W.surv);
    else
      hipLaunchKernelGGL(cand_compact_kernel<1>, dim3(grid), dim3(kThreads), 0, s, T, A, K, score_thresh, topk, W.st,
                         W.surv);
    JTSM_CHECK_LAUNCH("retinanet_candidates compact");
  }
  hipLaunchKernelGGL(cand_emit_kernel, dim3(segs), dim3(kThreads), 0, s, T, A, K, topk, W.st, W.surv, anchors, P,
                     scale_clamp, boxes, scores, classes, rows, counts);
  JTSM_CHECK_LAUNCH("retinanet_candidates emit");
  return JTSM_OK;
}

}  // extern "C"
