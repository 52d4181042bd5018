// Panoptic-DeepLab (projects/Panoptic-DeepLab/panoptic_deeplab/{panoptic_seg,post_processing}.py, train_net.py:100-124):
//   losses    centre (MSE) and offset (L1) regression of the bilinearly xS up-sampled stride-S predictions against
//             full-resolution targets, weighted per pixel and divided by the weights' sum.  One thread per output pixel
//             interpolates its one or two channels on the fly (bilinear_ce.h: lerp_scale, bilerp); fp64 sums over fixed
//             chunks in a fixed order (reduce.h: wg_tree_sum, fold_chunks); the backward is a gather per source pixel
//             that forms the same interpolated value again.  sum(w) == 0 is decided on the device: loss and gradient
//             exactly 0.
//   centres   find_instance_center: threshold, k x k max-pool NMS (separable, one LDS tile per workgroup), the top_k-th
//             largest value of the suppressed map by the chunked radix select of select.h (key order: its header), then
//             an ordered compaction of the pixels STRICTLY above max(that value, 0): row-major order, at most
//             top_k - 1 of them, none of those tied with the cut.
//   grouping  group_pixels: per pixel the arg-min over the centres (in LDS) of sqrtf(dy*dy + dx*dx); the lowest centre
//             index wins equal distances.  No K x HW intermediate.
//   merge     merge_semantic_and_instance: K x C class histogram (integer atomics), majority class per instance (the
//             smallest class on equal counts, torch.mode's rule), ids handed out in ascending instance order with a
//             counter per class, stuff classes by area, the (n,5) segment table, and per thing segment the box, the mean
//             soft-max probability of its class (fp64 per pixel, summed as 32.32 fixed point with integer atomics) and
//             the centre heat at the truncated mean pixel (exact integer coordinate sums divided in fp64).
//   adam      torch.optim.Adam (L2 decay added to the gradient, no amsgrad) over many tensors in one launch.
// Built with -ffp-contract=off: every product and sum below rounds as written.
#include <climits>

#include "bilinear_ce.h"
#include "common.h"
#include "reduce.h"
#include "select.h"
#include "workspace.h"

namespace jtsm {
namespace {

constexpr int PD_THREADS = kChunkThreads;     // the chunked passes (select.h) and every other kernel alike
constexpr int PD_MAX_CENTERS = 1024;    // centres held in LDS by the grouping kernel (the reference's top_k is 200)
constexpr int PD_MAX_CLASSES = 64;
constexpr int PD_TILE_H = 16, PD_TILE_W = 64, PD_MAX_PAD = 15;     // NMS tile; nms_kernel <= 31
constexpr int PD_HIST_LDS_CELLS = 16000;                           // K x C + C counters that fit a 64 KB LDS histogram

struct Min2 { __device__ int operator()(int a, int b) const { return a < b ? a : b; } };

// ---------------------------------------------------------------------------------------------------------------------
// losses
// ---------------------------------------------------------------------------------------------------------------------
// part[b] = {sum of loss * w, sum of w} of chunk b in fp64.  kind 0: (up - t)^2, kind 1: |S * up - t| summed over C.
__global__ __launch_bounds__(PD_THREADS) void pd_loss_fwd_kernel(const float* __restrict__ pred, int ld, int C,
                                                                 const float* __restrict__ target,
                                                                 const float* __restrict__ weights, int kind, long npix,
                                                                 long chunk, int Hs, int Ws, int S,
                                                                 double* __restrict__ part) {
  __shared__ double sl[PD_THREADS], sw[PD_THREADS];
  const int t = threadIdx.x;
  const int H = Hs * S, W = Ws * S;
  const long HW = (long)H * W;
  const float inv = 1.f / (float)S, mult = (float)S;
  const ChunkSpan ch = chunk_of_wg(npix, chunk);
  double accl = 0.0, accw = 0.0;
  for (long p = ch.p0 + t; p < ch.p1; p += PD_THREADS) {
    const int ow = (int)(p % W);
    const long q = p / W;
    const int oh = (int)(q % H), n = (int)(q / H);
    const float w = weights[p];
    accw += (double)w;
    const Lerp a = lerp_scale(oh, Hs, inv), b = lerp_scale(ow, Ws, inv);
    const float* zn = pred + (size_t)n * Hs * Ws * ld;
    const long o = (long)oh * W + ow;
    for (int c = 0; c < C; ++c) {
      const float up = bilerp(zn + c, ld, Ws, a, b);
      const float tv = target[((long)n * C + c) * HW + o];
      float l;
      if (kind == 0) { const float d = up - tv; l = d * d; }
      else l = fabsf(mult * up - tv);
      accl += (double)(l * w);
    }
  }
  wg_tree_sum<PD_THREADS>(accl, sl, accw, sw);
  if (t == 0) { part[2 * blockIdx.x] = accl; part[2 * blockIdx.x + 1] = accw; }
}

// out[0] = sum(loss * w) / sum(w), out[1] = 1 / sum(w); both 0 where sum(w) is not positive.  The fixed-order fold of
// reduce.h over the pairs.
__global__ __launch_bounds__(PD_THREADS) void pd_loss_finish_kernel(const double* __restrict__ part, int wgs,
                                                                    float* __restrict__ out) {
  __shared__ double sl[PD_THREADS], sw[PD_THREADS];
  double L, Wt;
  fold_chunks<PD_THREADS>(part, part + 1, 2, wgs, sl, sw, L, Wt);
  if (threadIdx.x == 0) {
    const bool live = Wt > 0.0;
    out[0] = live ? (float)(L / Wt) : 0.f;
    out[1] = live ? (float)(1.0 / Wt) : 0.f;
  }
}

// one thread per (source pixel, lane j < ld): lanes j >= C are written 0
__global__ __launch_bounds__(PD_THREADS) void pd_loss_bwd_kernel(const float* __restrict__ pred, int ld, int C,
                                                                 const float* __restrict__ target,
                                                                 const float* __restrict__ weights, int kind,
                                                                 const float* __restrict__ out,
                                                                 const float* __restrict__ upstream,
                                                                 float* __restrict__ dpred, int N, int Hs, int Ws, int S) {
  const long total = (long)N * Hs * Ws * ld;
  const int H = Hs * S, W = Ws * S;
  const long HW = (long)H * W;
  const float inv = 1.f / (float)S, mult = (float)S;
  const float inv_sum = out[1];
  const float k = (upstream ? *upstream : 1.f) * inv_sum;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % ld);
    if (c >= C || inv_sum == 0.f) { dpred[i] = 0.f; continue; }
    const long p = i / ld;
    const int w = (int)(p % Ws);
    const long q = p / Ws;
    const int h = (int)(q % Hs), n = (int)(q / Hs);
    const float* zc = pred + (size_t)n * Hs * Ws * ld + c;
    const float* tc = target + ((long)n * C + c) * HW;
    const float* wn = weights + (long)n * HW;
    const int oh0 = max(S * h - (S + 1) / 2, 0), oh1 = min(S * h + S + (S + 1) / 2, H);
    const int ow0 = max(S * w - (S + 1) / 2, 0), ow1 = min(S * w + S + (S + 1) / 2, W);
    float acc = 0.f;
    for (int oh = oh0; oh < oh1; ++oh) {
      const Lerp a = lerp_scale(oh, Hs, inv);
      const float wy = (a.i0 == h ? a.l0 : 0.f) + (a.i1 == h ? a.l1 : 0.f);
      if (wy == 0.f) continue;
      for (int ow = ow0; ow < ow1; ++ow) {
        const Lerp b = lerp_scale(ow, Ws, inv);
        const float wx = (b.i0 == w ? b.l0 : 0.f) + (b.i1 == w ? b.l1 : 0.f);
        if (wx == 0.f) continue;
        const long o = (long)oh * W + ow;
        const float wt = wn[o];
        if (wt == 0.f) continue;
        const float up = bilerp(zc, ld, Ws, a, b);
        const float tv = tc[o];
        float g;
        if (kind == 0) g = 2.f * (up - tv);
        else { const float d = mult * up - tv; g = d > 0.f ? mult : (d < 0.f ? -mult : 0.f); }
        acc = __fmaf_rn(wy * wx, g * wt, acc);
      }
    }
    dpred[i] = acc * k;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// centres
// ---------------------------------------------------------------------------------------------------------------------
// sup = x where x > threshold and x equals the maximum of its k x k window (padded with -inf, as F.max_pool2d), else -1
__global__ __launch_bounds__(PD_THREADS) void pd_nms_kernel(const float* __restrict__ heat, int H, int W, float threshold,
                                                            int pad, float* __restrict__ sup) {
  __shared__ float tile[(PD_TILE_H + 2 * PD_MAX_PAD) * (PD_TILE_W + 2 * PD_MAX_PAD)];
  __shared__ float rowmax[(PD_TILE_H + 2 * PD_MAX_PAD) * PD_TILE_W];
  const int t = threadIdx.x;
  const int y0 = blockIdx.y * PD_TILE_H, x0 = blockIdx.x * PD_TILE_W;
  const int th = PD_TILE_H + 2 * pad, tw = PD_TILE_W + 2 * pad, k = 2 * pad + 1;
  const float ninf = -__builtin_huge_valf();
  for (int i = t; i < th * tw; i += PD_THREADS) {
    const int y = y0 - pad + i / tw, x = x0 - pad + i % tw;
    float v = ninf;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      v = heat[(long)y * W + x];
      v = v > threshold ? v : -1.f;
    }
    tile[i] = v;
  }
  __syncthreads();
  for (int i = t; i < th * PD_TILE_W; i += PD_THREADS) {
    const int r = i / PD_TILE_W, c = i % PD_TILE_W;
    float m = ninf;
    for (int j = 0; j < k; ++j) m = fmaxf(m, tile[r * tw + c + j]);
    rowmax[i] = m;
  }
  __syncthreads();
  for (int i = t; i < PD_TILE_H * PD_TILE_W; i += PD_THREADS) {
    const int r = i / PD_TILE_W, c = i % PD_TILE_W;
    const int y = y0 + r, x = x0 + c;
    if (y >= H || x >= W) continue;
    float m = ninf;
    for (int j = 0; j < k; ++j) m = fmaxf(m, rowmax[(r + j) * PD_TILE_W + c]);
    const float v = tile[(r + pad) * tw + c + pad];
    sup[(long)y * W + x] = v == m ? v : -1.f;
  }
}

// kept: strictly above max(the top_k-th value, 0)
__device__ __forceinline__ unsigned pd_cut_key(const SelectState* __restrict__ st) {
  const unsigned zero = ordered_bits(0.f);
  return st->prefix > zero ? st->prefix : zero;
}

__global__ __launch_bounds__(PD_THREADS) void pd_keep_count_kernel(const float* __restrict__ sup, long n, long chunk,
                                                                   const SelectState* __restrict__ st,
                                                                   unsigned* __restrict__ cnt) {
  __shared__ unsigned slot[PD_THREADS / 64];
  const unsigned cut = pd_cut_key(st);
  const ChunkSpan ch = chunk_of_wg(n, chunk);
  unsigned c = 0u;
  for (long p = ch.p0 + threadIdx.x; p < ch.p1; p += PD_THREADS) c += ordered_bits(sup[p]) > cut ? 1u : 0u;
  c = wg_reduce<PD_THREADS / 64>(c, Add(), slot);
  if (threadIdx.x == 0) cnt[blockIdx.x] = c;
}

__global__ __launch_bounds__(PD_THREADS) void pd_keep_emit_kernel(const float* __restrict__ sup, long n, long chunk, int W,
                                                                  const SelectState* __restrict__ st,
                                                                  const unsigned* __restrict__ cnt, int wgs, int top_k,
                                                                  int* __restrict__ centers, int* __restrict__ count) {
  __shared__ unsigned slot[PD_THREADS / 64];
  __shared__ int wave_count[PD_THREADS / 64];
  const int t = threadIdx.x;
  const unsigned cut = pd_cut_key(st);
  unsigned before = 0u, all = 0u;
  for (int b = t; b < wgs; b += PD_THREADS) {
    const unsigned c = cnt[b];
    all += c;
    if (b < (int)blockIdx.x) before += c;
  }
  unsigned base = wg_reduce<PD_THREADS / 64>(before, Add(), slot);
  if (blockIdx.x == 0) {
    const unsigned total = wg_reduce<PD_THREADS / 64>(all, Add(), slot);
    const int kept = (int)(total < (unsigned)top_k ? total : (unsigned)top_k);
    if (t == 0) *count = kept;
    for (int r = kept + t; r < top_k; r += PD_THREADS) { centers[2 * r] = -1; centers[2 * r + 1] = -1; }
  }
  const ChunkSpan ch = chunk_of_wg(n, chunk);
  for (long q = ch.p0; q < ch.p1; q += PD_THREADS) {      // (uniform trip count: the compaction has barriers)
    const long p = q + t;
    const bool keep = p < ch.p1 && ordered_bits(sup[p]) > cut;
    int total;
    const int s = compact_wg<PD_THREADS / 64>(keep, wave_count, total);
    const unsigned row = base + (unsigned)s;
    if (keep && row < (unsigned)top_k) {
      centers[2 * row] = (int)(p / W);
      centers[2 * row + 1] = (int)(p % W);
    }
    base += (unsigned)total;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// semantic arg-max and grouping
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PD_THREADS) void pd_argmax_kernel(const float* __restrict__ logits, int C, long HW,
                                                               int* __restrict__ sem) {
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += (long)gridDim.x * blockDim.x) {
    float best = logits[p];
    int bi = 0;
    for (int c = 1; c < C; ++c) {
      const float v = logits[(long)c * HW + p];
      if (v > best) { best = v; bi = c; }
    }
    sem[p] = bi;
  }
}

// ins = (arg-min over the centres of sqrtf(dy*dy + dx*dx) + 1) * thing; 0 everywhere without a centre.  thing: the
// look-up table of the pixel's class where sem != NULL, else 1.  The square root is taken only where the squared
// distance is smaller than the best one's (the root is monotone, so no other centre can be strictly nearer).
__global__ __launch_bounds__(PD_THREADS) void pd_group_kernel(const int* __restrict__ centers, const int* __restrict__ count,
                                                              int max_centers, const float* __restrict__ offsets,
                                                              const int* __restrict__ sem,
                                                              const unsigned char* __restrict__ thing_lut, int C,
                                                              int* __restrict__ ins, int H, int W) {
  __shared__ float cy[PD_MAX_CENTERS], cx[PD_MAX_CENTERS];
  int K = *count;
  K = K < max_centers ? K : max_centers;
  K = K < 0 ? 0 : K;
  for (int i = threadIdx.x; i < K; i += PD_THREADS) { cy[i] = (float)centers[2 * i]; cx[i] = (float)centers[2 * i + 1]; }
  __syncthreads();
  const long HW = (long)H * W;
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += (long)gridDim.x * blockDim.x) {
    int id = 0;
    bool thing = true;
    if (sem) { const int s = sem[p]; thing = s >= 0 && s < C && thing_lut[s] != 0; }
    if (K > 0 && thing) {
      const float ly = (float)(int)(p / W) + offsets[p], lx = (float)(int)(p % W) + offsets[HW + p];
      float dy = cy[0] - ly, dx = cx[0] - lx;
      float best2 = dy * dy + dx * dx, best = sqrtf(best2);
      int bi = 0;
      for (int k = 1; k < K; ++k) {
        dy = cy[k] - ly; dx = cx[k] - lx;
        const float d2 = dy * dy + dx * dx;
        if (d2 < best2) {
          const float d = sqrtf(d2);
          if (d < best) { best = d; best2 = d2; bi = k; }
        }
      }
      id = bi + 1;
    }
    ins[p] = id;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// merge
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool pd_is_thing(int i, int s, const unsigned char* __restrict__ thing_seg,
                                            const unsigned char* __restrict__ thing_lut, int C, long p) {
  if (i <= 0) return false;
  if (thing_seg) return thing_seg[p] != 0;
  return s >= 0 && s < C && thing_lut[s] != 0;
}

// hist[(i - 1) * C + s] += 1 for thing pixels of instance i, stuff[s] += 1 for pixels outside every instance.  LDS:
// K * C + C counters per workgroup (dynamic), flushed with one global atomic per non-zero counter; lds == 0: global atomics.
__global__ __launch_bounds__(PD_THREADS) void pd_hist_kernel(const int* __restrict__ sem, const int* __restrict__ ins,
                                                             const unsigned char* __restrict__ thing_seg,
                                                             const unsigned char* __restrict__ thing_lut, int K, int C,
                                                             long HW, long chunk, int lds, int* __restrict__ hist,
                                                             int* __restrict__ stuff) {
  extern __shared__ int cells[];
  const int ncell = K * C + C;
  if (lds) {
    for (int i = threadIdx.x; i < ncell; i += PD_THREADS) cells[i] = 0;
    __syncthreads();
  }
  const ChunkSpan ch = chunk_of_wg(HW, chunk);
  for (long p = ch.p0 + threadIdx.x; p < ch.p1; p += PD_THREADS) {
    const int s = sem[p], i = ins[p];
    if (s < 0 || s >= C || i < 0 || i > K) continue;
    int cell = -1;
    if (i == 0) cell = K * C + s;
    else if (pd_is_thing(i, s, thing_seg, thing_lut, C, p)) cell = (i - 1) * C + s;
    if (cell < 0) continue;
    if (lds) atomicAdd(&cells[cell], 1);
    else atomicAdd(cell < K * C ? &hist[cell] : &stuff[cell - K * C], 1);
  }
  if (lds) {
    __syncthreads();
    for (int i = threadIdx.x; i < ncell; i += PD_THREADS) {
      const int v = cells[i];
      if (v) atomicAdd(i < K * C ? &hist[i] : &stuff[i - K * C], v);
    }
  }
}

struct PdSegStat { unsigned long long sum_y, sum_x, prob; int x0, y0, x1, y1; };

// One wavefront.  Lanes: majority class (smallest on equal counts) and area per instance; lane 0: the walk in ascending
// instance order with a counter per class, then the stuff classes in ascending order.
// table rows {id, isthing, category, instance_id, area}; ins_row[i - 1] = row of instance i or -1; stuff_ok[c].
__global__ __launch_bounds__(64) void pd_walk_kernel(const int* __restrict__ hist, const int* __restrict__ stuff,
                                                     const unsigned char* __restrict__ thing_lut, int K, int C,
                                                     int label_divisor, int stuff_area, int id_offset,
                                                     int* __restrict__ table, int* __restrict__ num,
                                                     int* __restrict__ ins_row, int* __restrict__ stuff_ok,
                                                     PdSegStat* __restrict__ stat) {
  __shared__ int mode[PD_MAX_CENTERS], area[PD_MAX_CENTERS];
  __shared__ int counter[PD_MAX_CLASSES];
  const int lane = threadIdx.x;
  for (int k = lane; k < K; k += 64) {
    int tot = 0, bestc = 0, m = 0;
    for (int c = 0; c < C; ++c) {
      const int v = hist[k * C + c];
      tot += v;
      if (v > bestc) { bestc = v; m = c; }
    }
    mode[k] = m; area[k] = tot;
    PdSegStat z;
    z.sum_y = 0ull; z.sum_x = 0ull; z.prob = 0ull; z.x0 = INT_MAX; z.y0 = INT_MAX; z.x1 = -1; z.y1 = -1;
    stat[k] = z;
  }
  if (lane < PD_MAX_CLASSES) counter[lane] = 0;
  __syncthreads();
  if (lane == 0) {
    int n = 0;
    for (int k = 0; k < K; ++k) {
      if (area[k] <= 0) { ins_row[k] = -1; continue; }
      const int m = mode[k], id = ++counter[m];
      ins_row[k] = n;
      int* r = table + 5 * n;
      r[0] = m * label_divisor + id + id_offset; r[1] = 1; r[2] = m; r[3] = id; r[4] = area[k];
      ++n;
    }
    num[1] = n;                     // thing rows
    for (int c = 0; c < C; ++c) {
      const int a = stuff[c];
      const bool ok = thing_lut[c] == 0 && a > 0 && a >= stuff_area;
      stuff_ok[c] = ok ? 1 : 0;
      if (ok) {
        int* r = table + 5 * n;
        r[0] = c * label_divisor + id_offset; r[1] = 0; r[2] = c; r[3] = -1; r[4] = a;
        ++n;
      }
    }
    num[0] = n;
  }
}

// the panoptic map, and (logits != NULL) per thing segment: coordinate sums, box extremes and the 32.32 fixed-point sum
// of the soft-max probability of the segment's class.  stat is indexed by instance (ins - 1), as pd_inst_kernel reads it.
// Per-pixel atomics would pile up on a few addresses (seven per thing pixel on one record per instance), so every
// wavefront folds the lanes of each instance it holds and sends one set of atomics per instance.
__global__ __launch_bounds__(PD_THREADS) void pd_paint_kernel(const int* __restrict__ sem, const int* __restrict__ ins,
                                                              const unsigned char* __restrict__ thing_seg,
                                                              const unsigned char* __restrict__ thing_lut,
                                                              const float* __restrict__ logits, int K, int C, int H, int W,
                                                              int label_divisor, int void_label, int id_offset,
                                                              const int* __restrict__ table,
                                                              const int* __restrict__ ins_row,
                                                              const int* __restrict__ stuff_ok, int* __restrict__ pan,
                                                              PdSegStat* __restrict__ stat) {
  const long HW = (long)H * W;
  const long step = (long)gridDim.x * blockDim.x;
  const long rounds = (HW + step - 1) / step;
  for (long it = 0; it < rounds; ++it) {         // (uniform trip count: the wavefront folds need every lane)
    const long p = it * step + (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = p < HW;
    int row = -1, key = -1, y = 0, x = 0;     // table row; instance index (stat is kept per instance) or -1
    unsigned long long pf = 0ull;
    if (in) {
      const int s = sem[p], i = ins[p];
      int label = void_label + id_offset;
      if (s >= 0 && s < C && i >= 0 && i <= K) {
        if (i == 0) {
          if (stuff_ok[s]) label = s * label_divisor + id_offset;
        } else if (pd_is_thing(i, s, thing_seg, thing_lut, C, p)) {
          row = ins_row[i - 1];
          if (row >= 0) { label = table[5 * row]; key = i - 1; }
        }
      }
      pan[p] = label;
      if (row >= 0 && logits) {
        y = (int)(p / W); x = (int)(p % W);
        const int cls = table[5 * row + 2];
        float mx = logits[p];
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, logits[(long)c * HW + p]);
        double sum = 0.0, mine = 0.0;
        for (int c = 0; c < C; ++c) {
          const double e = exp((double)logits[(long)c * HW + p] - (double)mx);
          sum += e;
          if (c == cls) mine = e;
        }
        pf = __double2ull_rn(mine / sum * 4294967296.0);
      }
    }
    if (!logits) continue;
    // one set of atomics per (wavefront, instance): the lanes of each instance present in the wavefront fold first
    unsigned long long todo = __ballot(key >= 0);
    while (todo) {                               // (uniform: todo is the same in every lane)
      const int k = __shfl(key, __ffsll((long long)todo) - 1);
      const bool mine = key == k;
      const unsigned long long sy = wave_sum(mine ? (unsigned long long)y : 0ull);
      const unsigned long long sx = wave_sum(mine ? (unsigned long long)x : 0ull);
      const unsigned long long sp = wave_sum(mine ? pf : 0ull);
      const int x0 = wave_reduce(mine ? x : INT_MAX, Min2()), y0 = wave_reduce(mine ? y : INT_MAX, Min2());
      const int x1 = wave_reduce(mine ? x : -1, Max()), y1 = wave_reduce(mine ? y : -1, Max());
      if ((threadIdx.x & 63) == 0) {
        PdSegStat* st = stat + k;
        atomicAdd(&st->sum_y, sy); atomicAdd(&st->sum_x, sx); atomicAdd(&st->prob, sp);
        atomicMin(&st->x0, x0); atomicMin(&st->y0, y0); atomicMax(&st->x1, x1); atomicMax(&st->y1, y1);
      }
      todo &= ~__ballot(mine);
    }
  }
}

// inst row r (thing rows only): {x0, y0, x1 + 1, y1 + 1, mean class probability, centre heat, centre y, centre x}
__global__ __launch_bounds__(PD_THREADS) void pd_inst_kernel(const int* __restrict__ table, const int* __restrict__ num,
                                                             const int* __restrict__ ins_row, int K,
                                                             const PdSegStat* __restrict__ stat,
                                                             const float* __restrict__ heat, int H, int W,
                                                             float* __restrict__ inst) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const int r = ins_row[k];
  if (r < 0 || r >= num[1]) return;
  const PdSegStat s = stat[k];
  const double area = (double)table[5 * r + 4];
  int cy = (int)((double)s.sum_y / area), cx = (int)((double)s.sum_x / area);
  cy = cy < 0 ? 0 : (cy >= H ? H - 1 : cy);
  cx = cx < 0 ? 0 : (cx >= W ? W - 1 : cx);
  float* o = inst + 8 * r;
  o[0] = (float)s.x0; o[1] = (float)s.y0; o[2] = (float)(s.x1 + 1); o[3] = (float)(s.y1 + 1);
  o[4] = (float)((double)s.prob / 4294967296.0 / area);
  o[5] = heat[(long)cy * W + cx];
  o[6] = (float)cy; o[7] = (float)cx;
}

// (hist | stuff: one memset clears both, up to `cleared`)
struct PdMergeWs { int* hist; int* stuff; size_t cleared; int* ins_row; int* stuff_ok; PdSegStat* stat; };
PdMergeWs carve_merge(Arena& a, int K, int C) {
  PdMergeWs M;
  M.hist = a.take<int>((size_t)K * C);
  M.stuff = a.take<int>(C);
  M.cleared = a.mark();
  M.ins_row = a.take<int>(K);
  M.stuff_ok = a.take<int>(C);
  M.stat = a.take<PdSegStat>(K);
  return M;
}

struct PdCenterWs { float* sup; unsigned* hist; SelectState* st; unsigned* cnt; };
PdCenterWs carve_centers(Arena& a, long HW) {
  PdCenterWs Cw;
  Cw.sup = a.take<float>((size_t)HW);
  Cw.hist = a.take<unsigned>(kMaxChunkWgs * kSelectBins);
  Cw.st = a.take<SelectState>(1);
  Cw.cnt = a.take<unsigned>(kMaxChunkWgs);
  return Cw;
}

inline int pd_grid(long n) { long b = (n + PD_THREADS - 1) / PD_THREADS; return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b)); }

// ---------------------------------------------------------------------------------------------------------------------
// Adam
// ---------------------------------------------------------------------------------------------------------------------
// Table rows are ten 64-bit words: {param, grad, exp_avg, exp_avg_sq, n, first_block, then pairs of float bit patterns
// (low | high << 32): (weight_decay | 1 - beta1), (beta2 | 1 - beta2), (eps | lr / bias_correction1),
// (sqrt(bias_correction2) | 0)}.
constexpr int ADAM_WG_ELEMS = 4096;     // elements a workgroup of 256 owns: one table search per four float4 rounds
struct AdamEntry { float* p; const float* g; float* m; float* v; long n; long first_block; unsigned long long w[4]; };
__device__ __forceinline__ float pd_lo(unsigned long long w) { return __uint_as_float((unsigned)(w & 0xffffffffull)); }
__device__ __forceinline__ float pd_hi(unsigned long long w) { return __uint_as_float((unsigned)(w >> 32)); }

// one element: every product, quotient and sum rounded as torch's kernels round them
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float wd, float omb1, float b2, float omb2,
                                         float eps, float step_size, float bc2s) {
  if (wd != 0.f) g = g + wd * p;
  m = m + omb1 * (g - m);
  v = v * b2 + omb2 * g * g;
  const float denom = sqrtf(v) / bc2s + eps;
  p = p - step_size * (m / denom);
}

__global__ __launch_bounds__(256) void adam_multi_kernel(const AdamEntry* __restrict__ tab, int nent) {
  int lo = 0, hi = nent - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].first_block <= (long)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const AdamEntry t = tab[lo];
  const float wd = pd_lo(t.w[0]), omb1 = pd_hi(t.w[0]), b2 = pd_lo(t.w[1]), omb2 = pd_hi(t.w[1]);
  const float eps = pd_lo(t.w[2]), step_size = pd_hi(t.w[2]), bc2s = pd_lo(t.w[3]);
  const bool aligned = (((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 15) == 0;
  const long first = ((long)blockIdx.x - t.first_block) * ADAM_WG_ELEMS + threadIdx.x * 4;
#pragma unroll
  for (int r = 0; r < ADAM_WG_ELEMS / 1024; ++r) {
    const long base = first + r * 1024;
    if (base >= t.n) return;
    if (base + 4 <= t.n && aligned) {
      float4 p = *reinterpret_cast<const float4*>(t.p + base);
      const float4 g = *reinterpret_cast<const float4*>(t.g + base);
      float4 m = *reinterpret_cast<const float4*>(t.m + base), v = *reinterpret_cast<const float4*>(t.v + base);
      adam_one(p.x, g.x, m.x, v.x, wd, omb1, b2, omb2, eps, step_size, bc2s);
      adam_one(p.y, g.y, m.y, v.y, wd, omb1, b2, omb2, eps, step_size, bc2s);
      adam_one(p.z, g.z, m.z, v.z, wd, omb1, b2, omb2, eps, step_size, bc2s);
      adam_one(p.w, g.w, m.w, v.w, wd, omb1, b2, omb2, eps, step_size, bc2s);
      *reinterpret_cast<float4*>(t.m + base) = m;
      *reinterpret_cast<float4*>(t.v + base) = v;
      *reinterpret_cast<float4*>(t.p + base) = p;
    } else {
      for (long i = base; i < t.n && i < base + 4; ++i) {
        float p = t.p[i], m = t.m[i], v = t.v[i];
        adam_one(p, t.g[i], m, v, wd, omb1, b2, omb2, eps, step_size, bc2s);
        t.m[i] = m; t.v[i] = v; t.p[i] = p;
      }
    }
  }
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" {

int jtsm_adam_block_elements(void) { return ADAM_WG_ELEMS; }

size_t jtsm_pdl_loss_workspace_bytes(void) { return a16(sizeof(double) * 2 * kMaxChunkWgs) + 16; }

static int pd_loss_check(int C, int ld, int kind, int N, int Hs, int Ws, int S, const char* what) {
  JTSM_REQUIRE(N >= 0 && Hs > 0 && Ws > 0 && S > 0 && C >= 1 && C <= 8 && ld >= C && (kind == 0 || kind == 1),
               "%s: need 1 <= C <= ld, C <= 8, kind 0 or 1 (C=%d ld=%d kind=%d)", what, C, ld, kind);
  JTSM_REQUIRE((long)N * Hs * S * Ws * S < (1L << 31) && (long)N * Hs * Ws * ld < (1L << 31),
               "%s: fewer than 2^31 pixels", what);
  return JTSM_OK;
}

int jtsm_pdl_loss_forward_f32(const float* pred, int ld, int C, const float* target, const float* weights, int kind,
                              float* out, void* workspace, int N, int Hs, int Ws, int S, void* stream) {
  int rc = pd_loss_check(C, ld, kind, N, Hs, Ws, S, "pdl_loss");
  if (rc) return rc;
  JTSM_REQUIRE(out && workspace && (N == 0 || (pred && target && weights)), "pdl_loss: null pointer");
  JTSM_REQUIRE(((uintptr_t)workspace & 7) == 0, "pdl_loss: workspace must be 8-byte aligned");
  hipStream_t st = as_stream(stream);
  const long npix = (long)N * Hs * S * Ws * S;
  const Chunks ch = chunks_of(npix);
  double* part = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(pd_loss_fwd_kernel, dim3(ch.wgs), dim3(PD_THREADS), 0, st, pred, ld, C, target, weights, kind, npix,
                     ch.chunk, Hs, Ws, S, part);
  hipLaunchKernelGGL(pd_loss_finish_kernel, dim3(1), dim3(PD_THREADS), 0, st, part, ch.wgs, out);
  JTSM_CHECK_LAUNCH("pdl_loss forward");
  return JTSM_OK;
}

int jtsm_pdl_loss_backward_f32(const float* pred, int ld, int C, const float* target, const float* weights, int kind,
                               const float* out, const float* upstream, float* dpred, int N, int Hs, int Ws, int S,
                               void* stream) {
  int rc = pd_loss_check(C, ld, kind, N, Hs, Ws, S, "pdl_loss backward");
  if (rc) return rc;
  if (N == 0) return JTSM_OK;
  JTSM_REQUIRE(pred && target && weights && out && dpred, "pdl_loss backward: null pointer");
  const long total = (long)N * Hs * Ws * ld;
  hipLaunchKernelGGL(pd_loss_bwd_kernel, dim3(pd_grid(total)), dim3(PD_THREADS), 0, as_stream(stream), pred, ld, C,
                     target, weights, kind, out, upstream, dpred, N, Hs, Ws, S);
  JTSM_CHECK_LAUNCH("pdl_loss backward");
  return JTSM_OK;
}

size_t jtsm_pdl_centers_workspace_bytes(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  Arena a{nullptr, false, 16};
  carve_centers(a, (long)H * W);
  return a.off + 16;
}

int jtsm_pdl_find_centers_f32(const float* heat, int H, int W, float threshold, int nms_kernel, int top_k, int* centers,
                              int* count, void* workspace, void* stream) {
  JTSM_REQUIRE(H > 0 && W > 0 && (long)H * W < (1L << 31), "pdl_find_centers: bad map size %d x %d", H, W);
  JTSM_REQUIRE(nms_kernel >= 1 && nms_kernel % 2 == 1 && nms_kernel <= 2 * PD_MAX_PAD + 1,
               "pdl_find_centers: nms_kernel must be odd and <= %d (got %d)", 2 * PD_MAX_PAD + 1, nms_kernel);
  JTSM_REQUIRE(top_k >= 1 && (long)top_k <= (long)H * W, "pdl_find_centers: need 1 <= top_k <= H*W (top_k=%d)", top_k);
  JTSM_REQUIRE(heat && centers && count && workspace, "pdl_find_centers: null pointer");
  JTSM_REQUIRE(((uintptr_t)workspace & 15) == 0, "pdl_find_centers: workspace must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const long HW = (long)H * W;
  Arena arena{static_cast<char*>(workspace), false, 16};
  const PdCenterWs Cw = carve_centers(arena, HW);
  const Chunks ch = chunks_of(HW);
  hipLaunchKernelGGL(pd_nms_kernel, dim3((W + PD_TILE_W - 1) / PD_TILE_W, (H + PD_TILE_H - 1) / PD_TILE_H),
                     dim3(PD_THREADS), 0, st, heat, H, W, threshold, (nms_kernel - 1) / 2, Cw.sup);
  launch_select(Cw.sup, HW, ch, (unsigned)top_k, Cw.st, Cw.hist, st);
  hipLaunchKernelGGL(pd_keep_count_kernel, dim3(ch.wgs), dim3(PD_THREADS), 0, st, Cw.sup, HW, ch.chunk, Cw.st, Cw.cnt);
  hipLaunchKernelGGL(pd_keep_emit_kernel, dim3(ch.wgs), dim3(PD_THREADS), 0, st, Cw.sup, HW, ch.chunk, W, Cw.st, Cw.cnt,
                     ch.wgs, top_k, centers, count);
  JTSM_CHECK_LAUNCH("pdl_find_centers");
  return JTSM_OK;
}

int jtsm_pdl_argmax_f32(const float* logits, int C, int H, int W, int* sem, void* stream) {
  JTSM_REQUIRE(C >= 1 && H > 0 && W > 0 && (long)H * W < (1L << 31) && logits && sem, "pdl_argmax: bad arguments");
  hipLaunchKernelGGL(pd_argmax_kernel, dim3(pd_grid((long)H * W)), dim3(PD_THREADS), 0, as_stream(stream), logits, C,
                     (long)H * W, sem);
  JTSM_CHECK_LAUNCH("pdl_argmax");
  return JTSM_OK;
}

int jtsm_pdl_group_pixels_f32(const int* centers, const int* count, int max_centers, const float* offsets, const int* sem,
                              const unsigned char* thing_lut, int num_classes, int* ins, int H, int W, void* stream) {
  JTSM_REQUIRE(H > 0 && W > 0 && (long)H * W < (1L << 31), "pdl_group_pixels: bad map size %d x %d", H, W);
  JTSM_REQUIRE(max_centers >= 0 && max_centers <= PD_MAX_CENTERS, "pdl_group_pixels: at most %d centres (got %d)",
               PD_MAX_CENTERS, max_centers);
  JTSM_REQUIRE(count && offsets && ins && (max_centers == 0 || centers), "pdl_group_pixels: null pointer");
  JTSM_REQUIRE(!sem || (thing_lut && num_classes >= 1), "pdl_group_pixels: a semantic map needs its thing table");
  hipLaunchKernelGGL(pd_group_kernel, dim3(pd_grid((long)H * W)), dim3(PD_THREADS), 0, as_stream(stream), centers, count,
                     max_centers, offsets, sem, thing_lut, num_classes, ins, H, W);
  JTSM_CHECK_LAUNCH("pdl_group_pixels");
  return JTSM_OK;
}

size_t jtsm_pdl_merge_workspace_bytes(int max_instances, int num_classes) {
  if (max_instances < 1 || max_instances > PD_MAX_CENTERS || num_classes < 1 || num_classes > PD_MAX_CLASSES) return 0;
  Arena a{nullptr, false, 16};
  carve_merge(a, max_instances, num_classes);
  return a.off + 16;
}

int jtsm_pdl_merge_f32(const int* sem, const int* ins, const unsigned char* thing_seg, const unsigned char* thing_lut,
                       const float* logits, const float* heat, int max_instances, int num_classes, int H, int W,
                       int label_divisor, int stuff_area, int void_label, int id_offset, int* pan, int* table, int* num,
                       float* inst, void* workspace, void* stream) {
  const int K = max_instances, C = num_classes;
  JTSM_REQUIRE(H > 0 && W > 0 && (long)H * W < (1L << 31), "pdl_merge: bad map size %d x %d", H, W);
  JTSM_REQUIRE(K >= 1 && K <= PD_MAX_CENTERS && C >= 1 && C <= PD_MAX_CLASSES,
               "pdl_merge: 1 <= instances <= %d, 1 <= classes <= %d (got %d, %d)", PD_MAX_CENTERS, PD_MAX_CLASSES, K, C);
  // (a class with label_divisor or more instances runs into the next class's ids, as in the reference: not checked,
  // the number of instances is known on the device only)
  JTSM_REQUIRE(label_divisor >= 1 && (long)C * label_divisor + K + 1 < (1L << 31),
               "pdl_merge: label_divisor %d with %d classes does not keep the ids in 32 bits", label_divisor, C);
  JTSM_REQUIRE(sem && ins && thing_lut && pan && table && num && workspace, "pdl_merge: null pointer");
  JTSM_REQUIRE((logits == nullptr) == (inst == nullptr) && (logits == nullptr) == (heat == nullptr),
               "pdl_merge: logits, heat and inst come together");
  JTSM_REQUIRE(((uintptr_t)workspace & 15) == 0, "pdl_merge: workspace must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const long HW = (long)H * W;
  Arena arena{static_cast<char*>(workspace), false, 16};
  const PdMergeWs M = carve_merge(arena, K, C);
  JTSM_CHECK_HIP(hipMemsetAsync(M.hist, 0, M.cleared, st));
  const Chunks ch = chunks_of(HW);
  const int ncell = K * C + C;
  const int lds = ncell <= PD_HIST_LDS_CELLS ? 1 : 0;
  hipLaunchKernelGGL(pd_hist_kernel, dim3(ch.wgs), dim3(PD_THREADS), lds ? sizeof(int) * ncell : 0, st, sem, ins,
                     thing_seg, thing_lut, K, C, HW, ch.chunk, lds, M.hist, M.stuff);
  hipLaunchKernelGGL(pd_walk_kernel, dim3(1), dim3(64), 0, st, M.hist, M.stuff, thing_lut, K, C, label_divisor,
                     stuff_area, id_offset, table, num, M.ins_row, M.stuff_ok, M.stat);
  hipLaunchKernelGGL(pd_paint_kernel, dim3(pd_grid(HW)), dim3(PD_THREADS), 0, st, sem, ins, thing_seg, thing_lut, logits,
                     K, C, H, W, label_divisor, void_label, id_offset, table, M.ins_row, M.stuff_ok, pan, M.stat);
  if (inst)
    hipLaunchKernelGGL(pd_inst_kernel, dim3((K + PD_THREADS - 1) / PD_THREADS), dim3(PD_THREADS), 0, st, table, num,
                       M.ins_row, K, M.stat, heat, H, W, inst);
  JTSM_CHECK_LAUNCH("pdl_merge");
  return JTSM_OK;
}

int jtsm_adam_multi_f32(const void* table, int entries, long blocks, void* stream) {
  JTSM_REQUIRE(entries >= 0 && blocks >= 0 && blocks < 2147483647L, "adam_multi: bad sizes");
  if (entries == 0 || blocks == 0) return JTSM_OK;
  JTSM_REQUIRE(table && ((uintptr_t)table & 15) == 0, "adam_multi: table must be a 16-byte aligned device pointer");
  hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const AdamEntry*>(table), entries);
  JTSM_CHECK_LAUNCH("adam_multi");
  return JTSM_OK;
}

}  // extern "C"
