// PointRend on the device: the point gather each way, the training point selection, the point loss
// each way and the inference subdivision step.  Built with -ffp-contract=off: which points are chosen and which side of
// 0.5 a target falls on hang on fp32 expressions written in the reference's order (point_features.py and ATen's
// grid_sample with align_corners=False and zero padding), every product and sum rounded.  No float atomics: every sum
// has a fixed order (the histogram of the radix select counts integers).
#include "bilinear_ce.h"
#include "common.h"
#include "reduce.h"
#include "select.h"
#include "sorted_segments.h"
#include "workspace.h"

namespace jtsm {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxLevels = 8;
constexpr int kMaxImages = 64;
constexpr int kMaxCandidates = 4096;      // selection: k * P keys of 8 bytes in LDS = 32 KB
constexpr int kSubThreads = 1024;
constexpr int kSubWaves = kSubThreads / kWave;
constexpr int kMaxTile = 112 * 112;       // subdivision: the H x W map in LDS, 49 KB
constexpr int kMaxChosen = 1024;          // subdivision: chosen cells of a roi, 8 KB of keys (the shipped N is 784)

// One source of the gather.  kind 0: a feature map shared by the rois of an image, indexed by the roi's image and read
// at the image-space point divided by (W, H) / scale.  kind 1: a map per roi (the coarse logits), indexed by the roi
// and read at the box-normalised point.  Strides in floats, so a channels-last map, a plain one and a channel slice of
// either are all described.
struct Levels {
  const float* map[kMaxLevels];
  long sn[kMaxLevels], sc[kMaxLevels], sy[kMaxLevels], sx[kMaxLevels];
  int H[kMaxLevels], W[kMaxLevels], C[kMaxLevels], col[kMaxLevels], kind[kMaxLevels];
  float scale[kMaxLevels];
  int L, Ctot, N;       // N: images behind the shared maps
};

// ATen's bilinear grid_sample tap (GridSampler.cuh): the north-west cell and the four weights nw, ne, sw, se.
struct Tap {
  float x0, y0;        // floor of the source coordinate, as floats (cast only once known to be inside)
  float w[4];
};

__device__ __forceinline__ float unnormalize(float p, int size) {
  const float g = 2.0f * p - 1.0f;                    // point_sample: 2.0 * point_coords - 1.0
  return ((g + 1.f) * (float)size - 1.f) / 2.f;       // grid_sampler_unnormalize, align_corners = false
}

__device__ __forceinline__ Tap tap_of(float px, float py, int W, int H) {
  const float ix = unnormalize(px, W), iy = unnormalize(py, H);
  Tap t;
  t.x0 = floorf(ix);
  t.y0 = floorf(iy);
  const float x1 = t.x0 + 1.f, y1 = t.y0 + 1.f;
  t.w[0] = (x1 - ix) * (y1 - iy);
  t.w[1] = (ix - t.x0) * (y1 - iy);
  t.w[2] = (x1 - ix) * (iy - t.y0);
  t.w[3] = (ix - t.x0) * (iy - t.y0);
  return t;
}

// cell `corner` (0 nw, 1 ne, 2 sw, 3 se) of a tap, if it lies inside the map (a NaN or a huge coordinate does not)
__device__ __forceinline__ bool tap_cell(const Tap& t, int corner, int W, int H, int& x, int& y) {
  const float fx = t.x0 + (float)(corner & 1), fy = t.y0 + (float)(corner >> 1);
  if (!(fx >= 0.f && fx <= (float)(W - 1) && fy >= 0.f && fy <= (float)(H - 1))) return false;
  x = (int)fx;
  y = (int)fy;
  return true;
}

// The box-normalised point of row (roi, q).  side == 0: read from `points`.  side > 0: cell q of the regular
// side x side grid (generate_regular_grid_point_coords), q in row-major order or, with `s2d`, in space-to-depth order
// ((by * side/2 + bx) * 2 + dy) * 2 + dx so that a 2x2 / stride-2 convolution over the grid is a 1x1 contraction.
__device__ __forceinline__ float2 point_of(const float* __restrict__ points, long row, int q, int side, int s2d) {
  if (side == 0) return make_float2(points[2 * row], points[2 * row + 1]);
  int x, y;
  if (s2d) {
    const int hb = side >> 1, blk = q >> 2;
    y = 2 * (blk / hb) + ((q >> 1) & 1);
    x = 2 * (blk % hb) + (q & 1);
  } else {
    y = q / side;
    x = q - y * side;
  }
  const float fs = (float)side;
  return make_float2(((float)(2 * x + 1) / fs - 1.f) * 0.5f + 0.5f, ((float)(2 * y + 1) / fs - 1.f) * 0.5f + 0.5f);
}

// get_point_coords_wrt_image: p * (x2 - x1) + x1, product and sum rounded
__device__ __forceinline__ float2 to_image(float2 p, const float* __restrict__ box) {
  float x = p.x * (box[2] - box[0]), y = p.y * (box[3] - box[1]);
  x = x + box[0];
  y = y + box[1];
  return make_float2(x, y);
}

// the normalised coordinate at which level l is read
__device__ __forceinline__ float2 level_point(const Levels& lv, int l, float2 p, float2 pim) {
  if (lv.kind[l]) return p;
  const float sx = (float)lv.W[l] / lv.scale[l], sy = (float)lv.H[l] / lv.scale[l];
  return make_float2(pim.x / sx, pim.y / sy);
}

// ---- a. gather, forward -----------------------------------------------------------------------------------------------
// One thread per (row, channel of some level); consecutive threads read consecutive channels.
__global__ __launch_bounds__(kThreads) void gather_forward_kernel(Levels lv, const float* __restrict__ boxes,
                                                                  const int* __restrict__ roi_image,
                                                                  const float* __restrict__ points, long total, int P,
                                                                  int side, int s2d, float* __restrict__ rows,
                                                                  long row_stride, float* __restrict__ coords) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const long row = i / lv.Ctot;
  int k = (int)(i - row * lv.Ctot);
  const int r = (int)(row / P), q = (int)(row - (long)r * P);
  int l = 0;
  while (l < lv.L - 1 && k >= lv.C[l]) { k -= lv.C[l]; ++l; }
  const float2 p = point_of(points, row, q, side, s2d);
  float2 pim = p;
  if (boxes) pim = to_image(p, boxes + 4 * (long)r);
  if (coords && i == row * lv.Ctot) { coords[2 * row] = pim.x; coords[2 * row + 1] = pim.y; }
  const float2 pl = level_point(lv, l, p, pim);
  const int W = lv.W[l], H = lv.H[l];
  const Tap t = tap_of(pl.x, pl.y, W, H);
  const long n = lv.kind[l] ? r : roi_image[r];
  const bool known = lv.kind[l] || (n >= 0 && n < lv.N);      // (a roi of no image reads zeros)
  const float* __restrict__ src = lv.map[l] + (known ? n : 0) * lv.sn[l] + (long)k * lv.sc[l];
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    int x, y;
    if (known && tap_cell(t, c, W, H, x, y)) acc += src[(long)y * lv.sy[l] + (long)x * lv.sx[l]] * t.w[c];
  }
  rows[row * row_stride + lv.col[l] + k] = acc;
}

// ---- b. gather, backward ----------------------------------------------------------------------------------------------
// Per-roi map (kind 1): one workgroup per roi; a cell (c, y, x) walks the roi's points in order.  The taps of 256
// points at a time sit in LDS.
__global__ __launch_bounds__(kThreads) void gather_backward_roi_kernel(const float* __restrict__ grad_rows,
                                                                       long row_stride, int col,
                                                                       const float* __restrict__ points, int P,
                                                                       int side, int s2d, int C, int H, int W,
                                                                       float* __restrict__ dmap, long sn, long sc,
                                                                       long sy, long sx) {
  __shared__ int tx[kThreads], ty[kThreads];
  __shared__ float tw[kThreads][4];
  const int r = blockIdx.x;
  const int cells = C * H * W;
  for (int base = 0; base < cells; base += kThreads) {
    const int cell = base + threadIdx.x;
    const int c = cell / (H * W), rem = cell - c * (H * W), y = rem / W, x = rem - y * W;
    float acc = 0.f;
    for (int p0 = 0; p0 < P; p0 += kThreads) {
      const int pn = min(kThreads, P - p0);
      __syncthreads();                       // the previous chunk's readers are done
      if ((int)threadIdx.x < pn) {
        const long row = (long)r * P + p0 + threadIdx.x;
        const float2 p = point_of(points, row, p0 + threadIdx.x, side, s2d);
        const Tap t = tap_of(p.x, p.y, W, H);
        // (a cell far outside compares unequal to every x, y below; clamp so that the cast is defined)
        tx[threadIdx.x] = (int)fminf(fmaxf(t.x0, -2.f), (float)W);
        ty[threadIdx.x] = (int)fminf(fmaxf(t.y0, -2.f), (float)H);
        if (!(t.x0 == t.x0)) tx[threadIdx.x] = -2;
        if (!(t.y0 == t.y0)) ty[threadIdx.x] = -2;
#pragma unroll
        for (int k = 0; k < 4; ++k) tw[threadIdx.x][k] = t.w[k];
      }
      __syncthreads();
      if (cell < cells) {
        for (int j = 0; j < pn; ++j) {
          const int dx = x - tx[j], dy = y - ty[j];
          if ((unsigned)dx <= 1u && (unsigned)dy <= 1u)
            acc += tw[j][dy * 2 + dx] * grad_rows[((long)r * P + p0 + j) * row_stride + col + c];
        }
      }
    }
    if (cell < cells) dmap[(long)r * sn + (long)c * sc + (long)y * sy + (long)x * sx] = acc;
  }
}

// Shared map (kind 0): one entry per (row, corner), keyed by the destination cell (image, y, x); entries without a
// cell get destination D and fall behind the last segment.
__global__ __launch_bounds__(kThreads) void gather_keys_kernel(const float* __restrict__ boxes,
                                                               const int* __restrict__ roi_image,
                                                               const float* __restrict__ points, long E, int P,
                                                               int side, int s2d, int N, int H, int W, float scale,
                                                               long D, int ebits, u64* __restrict__ keys,
                                                               int* __restrict__ vals) {
  const long e = (long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= E) return;
  const int corner = (int)(e & 3);
  const long row = e >> 2;
  const int r = (int)(row / P), q = (int)(row - (long)r * P);
  const float2 p = point_of(points, row, q, side, s2d);
  const float2 pim = to_image(p, boxes + 4 * (long)r);
  const float sx = (float)W / scale, sy = (float)H / scale;
  const Tap t = tap_of(pim.x / sx, pim.y / sy, W, H);
  long dest = D;
  int x, y;
  const int n = roi_image[r];
  if (n >= 0 && n < N && tap_cell(t, corner, W, H, x, y)) dest = ((long)n * H + y) * W + x;
  keys[e] = ((u64)dest << ebits) | (u64)e;
  vals[e] = __float_as_int(t.w[corner]);
}

// One workgroup per destination cell: its entries are start[d] .. start[d + 1] of the sorted list, ascending in e, and
// are summed in that order; lanes along the channels.  Every element of dmap is written, or, with `accumulate`,
// added to (one thread owns it: the order stays fixed).
__global__ __launch_bounds__(kThreads) void gather_walk_kernel(const float* __restrict__ grad_rows, long row_stride,
                                                               int col, const u64* __restrict__ keys,
                                                               const int* __restrict__ vals,
                                                               const int* __restrict__ start, int ebits, int C,
                                                               int accumulate, float* __restrict__ dmap) {
  const long d = blockIdx.x;
  const int beg = start[d], end = start[d + 1];
  const u64 emask = ((u64)1 << ebits) - 1;
  for (int c = threadIdx.x; c < C; c += kThreads) {
    float acc = 0.f;
    for (int j = beg; j < end; ++j) {
      const long row = (long)((keys[j] & emask) >> 2);
      acc += __int_as_float(vals[j]) * grad_rows[row * row_stride + col + c];
    }
    dmap[d * C + c] = accumulate ? dmap[d * C + c] + acc : acc;
  }
}

struct MapGradWs {
  long E, D;
  int ebits, dbits;
  u64 *key_a, *key_b;
  int *val_a, *val_b, *start;
  size_t cub_bytes;
  char* cub;
};

MapGradWs carve(Arena& a, long rows, long cells) {
  MapGradWs w;
  w.E = rows * 4;
  w.D = cells;
  w.ebits = bits_for(w.E > 0 ? w.E - 1 : 0);
  w.dbits = bits_for(w.D);
  w.key_a = a.take<u64>(w.E);
  w.key_b = a.take<u64>(w.E);
  w.val_a = a.take<int>(w.E);
  w.val_b = a.take<int>(w.E);
  w.start = a.take<int>(w.D + 2);
  w.cub_bytes = w.E > 0 ? sort_pairs_temp_bytes((int)w.E) : 0;
  w.cub = a.take<char>(w.cub_bytes);
  return w;
}

// ---- c. training point selection --------------------------------------------------------------------------------------
// One workgroup per roi.  Keys (uncertainty, candidate) in LDS; a candidate's place is the number of keys above its own.
__global__ __launch_bounds__(kThreads) void select_kernel(const float* __restrict__ coarse, int C, int S,
                                                          const long* __restrict__ classes,
                                                          const float* __restrict__ candidates, int K,
                                                          const float* __restrict__ randoms, int num_uncertain,
                                                          int P, float* __restrict__ out, int* __restrict__ chosen) {
  __shared__ unsigned long long key[kMaxCandidates];
  const int r = blockIdx.x;
  int ch = 0;
  if (C > 1) ch = (int)min(max(classes[r], 0L), (long)(C - 1));
  const float* __restrict__ src = coarse + ((long)r * C + ch) * S * S;
  const float* __restrict__ cand = candidates + (long)r * K * 2;
  for (int j = threadIdx.x; j < K; j += kThreads) {
    const Tap t = tap_of(cand[2 * j], cand[2 * j + 1], S, S);
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      int x, y;
      if (tap_cell(t, c, S, S, x, y)) acc += src[y * S + x] * t.w[c];
    }
    key[j] = order_key(-fabsf(acc), j);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < K; j += kThreads) {
    const unsigned long long mine = key[j];
    int before = 0;
    for (int i = 0; i < K; ++i) before += key[i] > mine ? 1 : 0;
    if (before < num_uncertain) {
      out[((long)r * P + before) * 2] = cand[2 * j];
      out[((long)r * P + before) * 2 + 1] = cand[2 * j + 1];
      if (chosen) chosen[(long)r * num_uncertain + before] = j;
    }
  }
  const int rest = P - num_uncertain;
  for (int j = threadIdx.x; j < 2 * rest; j += kThreads)
    out[((long)r * P + num_uncertain) * 2 + j] = randoms[(long)r * rest * 2 + j];
}

// ---- d. point loss ----------------------------------------------------------------------------------------------------
struct Masks {
  const unsigned char* ptr[kMaxImages];
  int h[kMaxImages], w[kMaxImages], count[kMaxImages];
  int N;
};

// workspace: targets[rows] | partial sums, one per workgroup | partial correct counts; the backward reads `targets`, the
// first buffer, from the workspace pointer itself
struct LossWs { float* targets; double* part_sum; int* part_correct; };
LossWs carve_loss(Arena& a, size_t rows) {
  const size_t parts = (rows + kThreads - 1) / kThreads;
  LossWs w;
  w.targets = a.take<float>(rows);
  w.part_sum = a.take<double>(parts);
  w.part_correct = a.take<int>(parts);
  return w;
}

__global__ __launch_bounds__(kThreads) void loss_forward_kernel(const float* __restrict__ logits, long ld, int C,
                                                                const long* __restrict__ classes, Masks m,
                                                                const int* __restrict__ roi_image,
                                                                const int* __restrict__ matched,
                                                                const float* __restrict__ coords, long rows, int P,
                                                                float* __restrict__ targets,
                                                                double* __restrict__ part_sum,
                                                                int* __restrict__ part_correct) {
  __shared__ double sd[kWaves];
  __shared__ int si[kWaves];
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  double term = 0.0;
  int correct = 0;
  if (i < rows) {
    const int r = (int)(i / P);
    const int n = roi_image[r];
    float t = 0.f;
    if (n >= 0 && n < m.N && m.count[n] > 0) {
      const int inst = min(max(matched[r], 0), m.count[n] - 1);
      const int w = m.w[n], h = m.h[n];
      const unsigned char* __restrict__ bits = m.ptr[n] + (long)inst * h * w;
      const Tap tp = tap_of(coords[2 * i] / (float)w, coords[2 * i + 1] / (float)h, w, h);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        int x, y;
        if (tap_cell(tp, c, w, h, x, y)) t += (bits[(long)y * w + x] ? 1.f : 0.f) * tp.w[c];
      }
    }
    targets[i] = t;
    int ch = 0;
    if (C > 1) ch = (int)min(max(classes[r], 0L), (long)(C - 1));
    const float x = logits[i * ld + ch];
    // binary_cross_entropy_with_logits: (1 - t) * x + max(-x, 0) + log(1 + exp(-|x|))
    const float l = (1.f - t) * x + (fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x))));
    term = (double)l;
    correct = ((x > 0.f) == ((int)t != 0)) ? 1 : 0;      // the reference casts the target to uint8: below 1.0 is 0
  }
  term = wg_reduce<kWaves>(term, Add(), sd);
  correct = wg_reduce<kWaves>(correct, Add(), si);
  if (threadIdx.x == 0) { part_sum[blockIdx.x] = term; part_correct[blockIdx.x] = correct; }
}

__global__ __launch_bounds__(kThreads) void loss_total_kernel(const double* __restrict__ part_sum,
                                                              const int* __restrict__ part_correct, int parts,
                                                              long rows, float* __restrict__ loss,
                                                              int* __restrict__ stats) {
  __shared__ double sd[kWaves];
  __shared__ int si[kWaves];
  double s = 0.0;
  int c = 0;
  for (int j = threadIdx.x; j < parts; j += kThreads) { s += part_sum[j]; c += part_correct[j]; }
  s = wg_reduce<kWaves>(s, Add(), sd);
  c = wg_reduce<kWaves>(c, Add(), si);
  if (threadIdx.x == 0) {
    *loss = rows > 0 ? (float)(s / (double)rows) : 0.f;
    if (stats) { stats[0] = c; stats[1] = (int)rows; }
  }
}

__global__ __launch_bounds__(kThreads) void loss_backward_kernel(const float* __restrict__ logits, long ld, int C,
                                                                 const long* __restrict__ classes,
                                                                 const float* __restrict__ targets, long rows, int P,
                                                                 const float* __restrict__ g, float* __restrict__ d,
                                                                 long ldd) {
  const long e = (long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= rows * C) return;
  const long i = e / C;
  const int c = (int)(e - i * C);
  int ch = 0;
  if (C > 1) ch = (int)min(max(classes[i / P], 0L), (long)(C - 1));
  float v = 0.f;
  if (c == ch) {
    const float x = logits[i * ld + c];
    v = (1.f / (1.f + expf(-x)) - targets[i]) * (*g / (float)rows);
  }
  d[i * ldd + c] = v;
}

// ---- e. subdivision ---------------------------------------------------------------------------------------------------
// F.interpolate(scale_factor=2, mode="bilinear", align_corners=False): lerp_scale at 1 / 2 along each axis
__device__ __forceinline__ float upsampled(const float* __restrict__ tile, int H, int W, int p) {
  const int OW = 2 * W;
  const int Y = p / OW, X = p - Y * OW;
  const Lerp a = lerp_scale(Y, H, 0.5f), b = lerp_scale(X, W, 0.5f);
  return blend(a, b, tile[a.i0 * W + b.i0], tile[a.i0 * W + b.i1], tile[a.i1 * W + b.i0], tile[a.i1 * W + b.i1]);
}

// One workgroup per roi.  The H x W map sits in LDS; the 2H x 2W values are formed from it on every pass.  The n most
// uncertain cells are found by a radix select over the four bytes of ordered_bits(-|v|) (one histogram in LDS; the bin
// rule is select.h's top_bin), ties at the cut going to the
// lower cell index, and put into (uncertainty descending, index ascending) by counting.  `direct`: `in` is a given
// (R, H, W) uncertainty map, read from memory and ranked as it is (get_uncertain_point_coords_on_grid on its own);
// nothing is up-sampled or written to `out`.
__device__ __forceinline__ unsigned cell_key(const float* __restrict__ tile, const float* __restrict__ given, int H,
                                             int W, int p, int direct) {
  return direct ? ordered_bits(given[p]) : ordered_bits(-fabsf(upsampled(tile, H, W, p)));
}

__global__ __launch_bounds__(kSubThreads) void subdivide_kernel(const float* __restrict__ in, int H, int W, int direct,
                                                                float* __restrict__ out, int n, float half_w,
                                                                float step_w, float half_h, float step_h,
                                                                long* __restrict__ indices,
                                                                float* __restrict__ coords) {
  __shared__ float tile[kMaxTile];
  __shared__ unsigned hist[256];
  __shared__ unsigned long long chosen[kMaxChosen];
  __shared__ int wave_count[kSubWaves];
  const int r = blockIdx.x;
  const int total = direct ? H * W : 4 * H * W, OW = direct ? W : 2 * W;
  const float* __restrict__ given = in + (long)r * H * W;
  if (!direct) {
    for (int e = threadIdx.x; e < H * W; e += kSubThreads) tile[e] = given[e];
    __syncthreads();
    for (int p = threadIdx.x; p < total; p += kSubThreads) out[(long)r * total + p] = upsampled(tile, H, W, p);
  }
  if (n <= 0) return;                                   // (uniform: the skip rule, only up-sample)
  unsigned prefix = 0, mask = 0, need = (unsigned)n;
  for (int shift = 24; shift >= 0; shift -= 8) {
    __syncthreads();                                    // the previous digit's readers are done
    if (threadIdx.x < 256) hist[threadIdx.x] = 0;
    __syncthreads();
    for (int p = threadIdx.x; p < total; p += kSubThreads) {
      const unsigned k = cell_key(tile, given, H, W, p, direct);
      if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    unsigned above;
    const int b = top_bin(hist, need, above);           // (every thread walks the same bins: uniform)
    need -= above;
    prefix |= (unsigned)b << shift;
    mask |= 255u << shift;
  }
  // keys above the cut, and the `need` lowest-index cells at the cut, in index order
  int seen = 0, filled = 0;
  for (int base = 0; base < total; base += kSubThreads) {
    const int p = base + threadIdx.x;
    const unsigned k = p < total ? cell_key(tile, given, H, W, p, direct) : 0u;
    const bool at = p < total && k == prefix;
    int n_at, n_take;
    const int slot_at = compact_wg<kSubWaves>(at, wave_count, n_at);
    const bool take = p < total && (k > prefix || (at && (unsigned)(seen + slot_at) < need));
    const int slot = compact_wg<kSubWaves>(take, wave_count, n_take);
    if (take && filled + slot < kMaxChosen) chosen[filled + slot] = index_key(k, (unsigned)p);
    seen += n_at;
    filled += n_take;
  }
  __syncthreads();
  const int m = min(filled, min(n, kMaxChosen));
  for (int j = threadIdx.x; j < m; j += kSubThreads) {
    const unsigned long long mine = chosen[j];
    int before = 0;
    for (int i = 0; i < m; ++i) before += chosen[i] > mine ? 1 : 0;
    const int p = (int)key_index(mine);
    const int Y = p / OW, X = p - Y * OW;
    indices[(long)r * n + before] = p;
    coords[((long)r * n + before) * 2] = half_w + (float)X * step_w;
    coords[((long)r * n + before) * 2 + 1] = half_h + (float)Y * step_h;
  }
}

__global__ __launch_bounds__(kThreads) void scatter_kernel(const float* __restrict__ logits, long ld, int C,
                                                           const long* __restrict__ classes,
                                                           const long* __restrict__ indices, long total, int n,
                                                           int cells, float* __restrict__ map) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const long r = i / n;
  int ch = 0;
  if (C > 1) ch = (int)min(max(classes[r], 0L), (long)(C - 1));
  const long p = indices[i];
  if (p >= 0 && p < cells) map[r * cells + p] = logits[i * ld + ch];
}

int fill_levels(Levels& lv, const char* who, const float* const* maps, const int64_t* geom, const float* scales, int L) {
  JTSM_REQUIRE(L >= 1 && L <= kMaxLevels && maps && geom && scales, "%s: %d levels (1..%d)", who, L, kMaxLevels);
  lv.L = L;
  lv.Ctot = 0;
  for (int l = 0; l < L; ++l) {
    const int64_t* g = geom + 9 * l;
    JTSM_REQUIRE(maps[l] && g[0] >= 1 && g[1] >= 1 && g[2] >= 1 && g[3] >= 0 && g[0] < (1 << 20) && g[1] < (1 << 20) &&
                     g[2] < (1 << 20) && (g[4] == 0 || g[4] == 1) && scales[l] > 0.f,
                 "%s: level %d: H=%ld W=%ld C=%ld col=%ld kind=%ld scale=%g", who, l, (long)g[0], (long)g[1],
                 (long)g[2], (long)g[3], (long)g[4], (double)scales[l]);
    lv.map[l] = maps[l];
    lv.H[l] = (int)g[0]; lv.W[l] = (int)g[1]; lv.C[l] = (int)g[2]; lv.col[l] = (int)g[3]; lv.kind[l] = (int)g[4];
    lv.sn[l] = g[5]; lv.sc[l] = g[6]; lv.sy[l] = g[7]; lv.sx[l] = g[8];
    lv.scale[l] = scales[l];
    lv.Ctot += lv.C[l];
  }
  return JTSM_OK;
}

int check_grid(const char* who, int P, int side, int s2d, const float* points) {
  JTSM_REQUIRE(side >= 0 && (side == 0 || (long)side * side == P), "%s: a %d x %d grid for P = %d", who, side, side, P);
  JTSM_REQUIRE(!s2d || (side > 0 && side % 2 == 0), "%s: space-to-depth order needs an even grid side, got %d", who, side);
  JTSM_REQUIRE(side > 0 || points, "%s: neither points nor a grid", who);
  return JTSM_OK;
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" {

int jtsm_point_gather_forward_f32(const float* const* maps, const int64_t* geom, const float* scales, int L,
                                  int num_images, const float* boxes, const int32_t* roi_image, const float* points,
                                  int R, int P, int grid_side, int space_to_depth, float* rows, int64_t row_stride,
                                  float* coords_wrt_image, void* stream) {
  JTSM_REQUIRE(R >= 0 && P >= 1, "point_gather: R=%d P=%d", R, P);
  if (R == 0) return JTSM_OK;
  Levels lv;
  if (int rc = fill_levels(lv, "point_gather", maps, geom, scales, L)) return rc;
  lv.N = num_images;
  if (int rc = check_grid("point_gather", P, grid_side, space_to_depth, points)) return rc;
  bool shared = false;
  for (int l = 0; l < L; ++l) {
    shared = shared || lv.kind[l] == 0;
    JTSM_REQUIRE(lv.col[l] + lv.C[l] <= row_stride, "point_gather: level %d writes columns %d..%d of rows of %ld", l,
                 lv.col[l], lv.col[l] + lv.C[l], (long)row_stride);
  }
  JTSM_REQUIRE(rows && (!shared || (boxes && roi_image)) && (!coords_wrt_image || boxes), "point_gather: null pointer");
  const long total = (long)R * P * lv.Ctot;
  JTSM_REQUIRE(total / kThreads < (1L << 31) - 1, "point_gather: %ld outputs", total);
  hipLaunchKernelGGL(gather_forward_kernel, dim3(ceil_div(total, kThreads)), dim3(kThreads), 0, as_stream(stream), lv,
                     boxes, roi_image, points, total, P, grid_side, space_to_depth, rows, (long)row_stride,
                     coords_wrt_image);
  JTSM_CHECK_LAUNCH("point_gather forward");
  return JTSM_OK;
}

int jtsm_point_gather_backward_roi_f32(const float* grad_rows, int64_t row_stride, int col, const float* points, int R,
                                       int P, int grid_side, int space_to_depth, int C, int H, int W, float* grad_map,
                                       int64_t stride_n, int64_t stride_c, int64_t stride_y, int64_t stride_x,
                                       void* stream) {
  JTSM_REQUIRE(R >= 0 && P >= 1 && C >= 1 && H >= 1 && W >= 1 && (long)C * H * W < (1L << 31) && col >= 0 &&
                   col + C <= row_stride,
               "point_gather_backward_roi: R=%d P=%d C=%d H=%d W=%d col=%d stride=%ld", R, P, C, H, W, col,
               (long)row_stride);
  if (R == 0) return JTSM_OK;
  if (int rc = check_grid("point_gather_backward_roi", P, grid_side, space_to_depth, points)) return rc;
  JTSM_REQUIRE(grad_rows && grad_map, "point_gather_backward_roi: null pointer");
  hipLaunchKernelGGL(gather_backward_roi_kernel, dim3((unsigned)R), dim3(kThreads), 0, as_stream(stream), grad_rows,
                     (long)row_stride, col, points, P, grid_side, space_to_depth, C, H, W, grad_map, (long)stride_n,
                     (long)stride_c, (long)stride_y, (long)stride_x);
  JTSM_CHECK_LAUNCH("point_gather backward roi");
  return JTSM_OK;
}

size_t jtsm_point_gather_backward_map_workspace_bytes(int R, int P, int N, int H, int W) {
  if (R < 0 || P < 1 || N < 0 || H < 1 || W < 1) return 0;
  Arena a{nullptr};
  carve(a, (long)R * P, (long)N * H * W);
  return a.off;
}

int jtsm_point_gather_backward_map_f32(const float* grad_rows, int64_t row_stride, int col, const float* boxes,
                                       const int32_t* roi_image, const float* points, int R, int P, int grid_side,
                                       int space_to_depth, int N, int H, int W, int C, float scale, float* grad_map,
                                       int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  JTSM_REQUIRE(R >= 0 && P >= 1 && N >= 0 && H >= 1 && W >= 1 && C >= 1 && scale > 0.f && col >= 0 &&
                   col + C <= row_stride,
               "point_gather_backward_map: R=%d P=%d N=%d H=%d W=%d C=%d col=%d stride=%ld", R, P, N, H, W, C, col,
               (long)row_stride);
  const long cells = (long)N * H * W, rows = (long)R * P;
  if (cells == 0) return JTSM_OK;
  JTSM_REQUIRE(grad_map, "point_gather_backward_map: null pointer");
  JTSM_REQUIRE(rows * 4 <= 2147483647L && cells < 2147483647L, "point_gather_backward_map: %ld taps / %ld cells do not fit 31 bits",
               rows * 4, cells);
  hipStream_t st = as_stream(stream);
  if (rows == 0) {
    if (!accumulate) JTSM_CHECK_HIP(hipMemsetAsync(grad_map, 0, sizeof(float) * (size_t)cells * C, st));
    return JTSM_OK;
  }
  if (int rc = check_grid("point_gather_backward_map", P, grid_side, space_to_depth, points)) return rc;
  JTSM_REQUIRE(grad_rows && boxes && roi_image, "point_gather_backward_map: null pointer");
  Arena arena{static_cast<char*>(workspace)};
  const MapGradWs w = carve(arena, rows, cells);
  JTSM_REQUIRE(workspace && workspace_bytes >= arena.off && ((size_t)workspace & 255) == 0,
               "point_gather_backward_map: workspace of %zu bytes (256-byte aligned) needed", arena.off);
  JTSM_REQUIRE(w.ebits + w.dbits <= 64, "point_gather_backward_map: key of %d + %d bits", w.dbits, w.ebits);
  hipLaunchKernelGGL(gather_keys_kernel, dim3(ceil_div(w.E, kThreads)), dim3(kThreads), 0, st, boxes, roi_image, points,
                     w.E, P, grid_side, space_to_depth, N, H, W, scale, w.D, w.ebits, w.key_a, w.val_a);
  JTSM_CHECK_LAUNCH("point_gather keys");
  // stable, and over the destination bits only: inside a cell the entries keep their emission order, e ascending
  size_t cub_bytes = w.cub_bytes;
  JTSM_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(w.cub, cub_bytes, w.key_a, w.key_b, w.val_a, w.val_b, (int)w.E,
                                                    w.ebits, w.ebits + w.dbits, st));
  hipLaunchKernelGGL(segment_starts_kernel, dim3(ceil_div(w.D + 1, 64)), dim3(64), 0, st, w.key_b, (int)w.E, (int)w.D,
                     w.ebits, w.start);
  JTSM_CHECK_LAUNCH("point_gather segments");
  hipLaunchKernelGGL(gather_walk_kernel, dim3((unsigned)w.D), dim3(kThreads), 0, st, grad_rows, (long)row_stride, col,
                     w.key_b, w.val_b, w.start, w.ebits, C, accumulate, grad_map);
  JTSM_CHECK_LAUNCH("point_gather walk");
  return JTSM_OK;
}

int jtsm_point_select_f32(const float* coarse_logits, int R, int C, int S, const int64_t* classes,
                          const float* candidates, int num_candidates, const float* randoms, int num_uncertain,
                          int P, float* point_coords, int32_t* chosen, void* stream) {
  JTSM_REQUIRE(R >= 0 && C >= 1 && S >= 1 && S <= 4096 && P >= 1 && num_uncertain >= 0 && num_uncertain <= P &&
                   num_candidates >= num_uncertain && num_candidates <= kMaxCandidates,
               "point_select: R=%d C=%d S=%d P=%d uncertain=%d candidates=%d (<= %d)", R, C, S, P, num_uncertain,
               num_candidates, kMaxCandidates);
  if (R == 0) return JTSM_OK;
  JTSM_REQUIRE(coarse_logits && point_coords && (C == 1 || classes) && (num_candidates == 0 || candidates) &&
                   (num_uncertain == P || randoms),
               "point_select: null pointer");
  hipLaunchKernelGGL(select_kernel, dim3((unsigned)R), dim3(kThreads), 0, as_stream(stream), coarse_logits, C, S,
                     (const long*)classes, candidates, num_candidates, randoms, num_uncertain, P, point_coords, chosen);
  JTSM_CHECK_LAUNCH("point_select");
  return JTSM_OK;
}

size_t jtsm_point_loss_workspace_bytes(int R, int P) {
  const size_t rows = (size_t)(R > 0 ? R : 0) * (size_t)(P > 0 ? P : 0);
  Arena a{nullptr};
  carve_loss(a, rows);
  return a.off + 256;
}

int jtsm_point_loss_forward_f32(const float* logits, int64_t ld, int R, int P, int C, const int64_t* classes,
                                const uint8_t* const* masks, const int32_t* mask_geom, int N, const int32_t* roi_image,
                                const int32_t* matched, const float* coords_wrt_image, float* loss, int32_t* stats,
                                void* workspace, void* stream) {
  JTSM_REQUIRE(R >= 0 && P >= 1 && C >= 1 && ld >= C && N >= 0 && N <= kMaxImages, "point_loss: R=%d P=%d C=%d ld=%ld N=%d (<= %d)",
               R, P, C, (long)ld, N, kMaxImages);
  JTSM_REQUIRE(loss && workspace, "point_loss: null pointer");
  const long rows = (long)R * P;
  JTSM_REQUIRE(rows < (1L << 31) - kThreads, "point_loss: %ld rows", rows);
  const int parts = ceil_div(rows, kThreads);
  Arena arena{static_cast<char*>(workspace)};
  const LossWs w = carve_loss(arena, (size_t)rows);
  if (rows) {
    JTSM_REQUIRE(logits && (C == 1 || classes) && roi_image && matched && coords_wrt_image && (N == 0 || (masks && mask_geom)),
                 "point_loss: null pointer");
    Masks m;
    m.N = N;
    for (int n = 0; n < N; ++n) {
      m.h[n] = mask_geom[3 * n]; m.w[n] = mask_geom[3 * n + 1]; m.count[n] = mask_geom[3 * n + 2];
      m.ptr[n] = masks[n];
      JTSM_REQUIRE(m.count[n] >= 0 && (m.count[n] == 0 || (m.ptr[n] && m.h[n] >= 1 && m.w[n] >= 1)),
                   "point_loss: image %d: %d masks of %d x %d", n, m.count[n], m.h[n], m.w[n]);
    }
    hipLaunchKernelGGL(loss_forward_kernel, dim3(parts), dim3(kThreads), 0, as_stream(stream), logits, (long)ld, C,
                       (const long*)classes, m, roi_image, matched, coords_wrt_image, rows, P, w.targets, w.part_sum,
                       w.part_correct);
    JTSM_CHECK_LAUNCH("point_loss forward");
  }
  hipLaunchKernelGGL(loss_total_kernel, dim3(1), dim3(kThreads), 0, as_stream(stream), w.part_sum, w.part_correct,
                     parts, rows, loss, stats);
  JTSM_CHECK_LAUNCH("point_loss total");
  return JTSM_OK;
}

int jtsm_point_loss_backward_f32(const float* logits, int64_t ld, int R, int P, int C, const int64_t* classes,
                                 const float* grad_loss, const void* workspace, float* grad_logits, int64_t grad_ld,
                                 void* stream) {
  JTSM_REQUIRE(R >= 0 && P >= 1 && C >= 1 && ld >= C && grad_ld >= C, "point_loss: R=%d P=%d C=%d ld=%ld", R, P, C, (long)ld);
  const long rows = (long)R * P;
  if (rows == 0) return JTSM_OK;
  JTSM_REQUIRE(logits && (C == 1 || classes) && grad_loss && workspace && grad_logits, "point_loss: null pointer");
  JTSM_REQUIRE(rows * C / kThreads < (1L << 31) - 1, "point_loss: %ld elements", rows * C);
  hipLaunchKernelGGL(loss_backward_kernel, dim3(ceil_div(rows * C, kThreads)), dim3(kThreads), 0, as_stream(stream),
                     logits, (long)ld, C, (const long*)classes, (const float*)workspace, rows, P, grad_loss,
                     grad_logits, (long)grad_ld);
  JTSM_CHECK_LAUNCH("point_loss backward");
  return JTSM_OK;
}

int jtsm_point_subdivide_f32(const float* map, int R, int H, int W, float* upsampled_map, int num_points,
                             int64_t* indices, float* point_coords, void* stream) {
  JTSM_REQUIRE(R >= 0 && H >= 1 && W >= 1 && (long)H * W <= kMaxTile && num_points >= 0 && num_points <= kMaxChosen,
               "point_subdivide: R=%d H=%d W=%d (H * W <= %d) points=%d (<= %d)", R, H, W, kMaxTile, num_points,
               kMaxChosen);
  if (R == 0) return JTSM_OK;
  const int n = num_points < 4 * H * W ? num_points : 4 * H * W;
  JTSM_REQUIRE(map && upsampled_map && (n == 0 || (indices && point_coords)), "point_subdivide: null pointer");
  // get_uncertain_point_coords_on_grid: the steps are Python doubles, the sum is formed in fp32
  const double step_w = 1.0 / (double)(2 * W), step_h = 1.0 / (double)(2 * H);
  hipLaunchKernelGGL(subdivide_kernel, dim3((unsigned)R), dim3(kSubThreads), 0, as_stream(stream), map, H, W, 0,
                     upsampled_map, n, (float)(step_w / 2.0), (float)step_w, (float)(step_h / 2.0), (float)step_h,
                     (long*)indices, point_coords);
  JTSM_CHECK_LAUNCH("point_subdivide");
  return JTSM_OK;
}

int jtsm_point_topk_grid_f32(const float* uncertainty_map, int R, int H, int W, int num_points, int64_t* indices,
                             float* point_coords, void* stream) {
  JTSM_REQUIRE(R >= 0 && H >= 1 && W >= 1 && (long)H * W < (1L << 30) && num_points >= 1 && num_points <= kMaxChosen &&
                   num_points <= (long)H * W,
               "point_topk_grid: R=%d H=%d W=%d points=%d (<= %d and <= H * W)", R, H, W, num_points, kMaxChosen);
  if (R == 0) return JTSM_OK;
  JTSM_REQUIRE(uncertainty_map && indices && point_coords, "point_topk_grid: null pointer");
  const double step_w = 1.0 / (double)W, step_h = 1.0 / (double)H;
  hipLaunchKernelGGL(subdivide_kernel, dim3((unsigned)R), dim3(kSubThreads), 0, as_stream(stream), uncertainty_map, H,
                     W, 1, (float*)nullptr, num_points, (float)(step_w / 2.0), (float)step_w, (float)(step_h / 2.0),
                     (float)step_h, (long*)indices, point_coords);
  JTSM_CHECK_LAUNCH("point_topk_grid");
  return JTSM_OK;
}

int jtsm_point_scatter_f32(const float* point_logits, int64_t ld, int R, int num_points, int C, const int64_t* classes,
                           const int64_t* indices, int cells, float* map, void* stream) {
  JTSM_REQUIRE(R >= 0 && num_points >= 0 && C >= 1 && ld >= C && cells >= 1, "point_scatter: R=%d points=%d C=%d ld=%ld cells=%d",
               R, num_points, C, (long)ld, cells);
  const long total = (long)R * num_points;
  if (total == 0) return JTSM_OK;
  JTSM_REQUIRE(point_logits && (C == 1 || classes) && indices && map, "point_scatter: null pointer");
  hipLaunchKernelGGL(scatter_kernel, dim3(ceil_div(total, kThreads)), dim3(kThreads), 0, as_stream(stream),
                     point_logits, (long)ld, C, (const long*)classes, indices, total, num_points, cells, map);
  JTSM_CHECK_LAUNCH("point_scatter");
  return JTSM_OK;
}

}  // extern "C"
