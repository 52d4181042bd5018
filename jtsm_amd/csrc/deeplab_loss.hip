// DeepLabCE, the hard-pixel-mining cross-entropy (projects/DeepLab/deeplab/loss.py:6-40), fused with the bilinear xS
// up-sampling that precedes it (projects/DeepLab/deeplab/semantic_seg.py: F.interpolate(..., scale_factor=
// common_stride, mode="bilinear", align_corners=False) in DeepLabV3PlusHead.losses / DeepLabV3Head.losses).  The
// reference materialises the up-sampled logits, the per-pixel losses, and sorts them (torch.topk); here
//   forward   one thread per output pixel interpolates its logits on the fly (bilinear_ce.h, the code of
//             semseg_ops.hip) and writes the log-sum-exp and the per-pixel loss, 4 B each (0 where the target is
//             ignored, times `weights` where given);
//   select    the k-th largest loss is found by a radix select on the loss's bit pattern: four passes over 8-bit
//             digits from the top.  Every workgroup owns a contiguous chunk of pixels and counts its digits in LDS
//             (one histogram per wavefront: losses that crowd around log C early in training hit the same bin, and
//             global histogram atomics serialise there); one workgroup folds the per-workgroup histograms and picks
//             the bin.  The key orders every float: -0 = +0, every NaN on top (ordered_bits, common.h), so a NaN loss
//             is among the chosen and the result is NaN, as with torch.topk.  Nothing is read back; the workspace is
//             the histograms and one word per workgroup, whatever the number of pixels;
//   loss      (sum of the losses above the cut t + (k - their number) * t) / k, fp64 sums in a fixed order;
//   coef      the backward's per-pixel factor, selected * weight / k.  TIES AT THE CUT: of the pixels whose loss equals
//             t, those with the LOWER FLAT INDEX (n, h, w) are chosen first (the reference's topk leaves that open; the
//             rule is jtsm_retinanet_candidates_f32's).  Their ranks come from an ordered count: per-workgroup tie
//             counts, an exclusive scan over the workgroups, an ordered compaction inside each chunk;
//   backward  the deterministic gather of semseg_ops.hip with `coef` in place of the single upstream scalar.
// k is the caller's (int(top_k_percent_pixels * numel) in host doubles, numel counting ignored pixels too).
#include "bilinear_ce.h"
#include "common.h"
#include "reduce.h"

namespace jtsm {
namespace {

constexpr int DL_THREADS = 256;
constexpr int DL_MAX_WG = 512;         // workgroups of the select passes
constexpr int DL_SEL_SLICES = 4;       // slices of the per-workgroup histograms one select workgroup folds side by side
constexpr int DL_BINS = 256;           // 8-bit digits

struct DlState {
  unsigned prefix;      // digits chosen so far (high bits of the cut's key)
  unsigned need;        // how many of the elements that match the prefix are still to be taken
  unsigned ties;        // after the last pass: elements equal to the cut
  unsigned pad;
};

struct DlWs {
  unsigned* hist;       // [DL_MAX_WG][DL_BINS]
  DlState* st;
  unsigned* tie_count;  // [DL_MAX_WG]
  unsigned* tie_base;   // [DL_MAX_WG]
  double* sums;         // [DL_MAX_WG]
};
inline size_t a16(size_t b) { return (b + 15) & ~(size_t)15; }
inline size_t dl_ws_bytes() {
  return a16(sizeof(unsigned) * DL_MAX_WG * DL_BINS) + a16(sizeof(DlState)) + 2 * a16(sizeof(unsigned) * DL_MAX_WG) +
         a16(sizeof(double) * DL_MAX_WG) + 16;
}
inline DlWs dl_carve(void* workspace) {
  char* w = reinterpret_cast<char*>(workspace);
  DlWs W;
  W.hist = reinterpret_cast<unsigned*>(w); w += a16(sizeof(unsigned) * DL_MAX_WG * DL_BINS);
  W.st = reinterpret_cast<DlState*>(w); w += a16(sizeof(DlState));
  W.tie_count = reinterpret_cast<unsigned*>(w); w += a16(sizeof(unsigned) * DL_MAX_WG);
  W.tie_base = reinterpret_cast<unsigned*>(w); w += a16(sizeof(unsigned) * DL_MAX_WG);
  W.sums = reinterpret_cast<double*>(w);
  return W;
}

// chunk of workgroup b: pixels [b * chunk, min(npix, (b + 1) * chunk)), chunk a multiple of DL_THREADS
struct DlChunks { int wgs; long chunk; };
inline DlChunks dl_chunks(long npix) {
  DlChunks c;
  long tiles = (npix + DL_THREADS - 1) / DL_THREADS;
  long per = (tiles + DL_MAX_WG - 1) / DL_MAX_WG;
  if (per < 1) per = 1;
  c.chunk = per * DL_THREADS;
  c.wgs = (int)((npix + c.chunk - 1) / c.chunk);
  if (c.wgs < 1) c.wgs = 1;
  return c;
}

__global__ __launch_bounds__(DL_THREADS) void dl_fwd_kernel(const float* __restrict__ z, int ldc, int C,
                                                            const long* __restrict__ target,
                                                            const float* __restrict__ weights, float* __restrict__ lse,
                                                            float* __restrict__ pixel_loss, int N, int Hs, int Ws, int S,
                                                            long ignore) {
  const int H = Hs * S, W = Ws * S;
  const long npix = (long)N * H * W;
  const float inv = 1.f / (float)S;
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
    const long t = target[p];
    const int ow = (int)(p % W);
    const long q = p / W;
    const int oh = (int)(q % H), n = (int)(q / H);
    float vt;
    const float l = ce_pixel_lse(z, ldc, C, n, oh, ow, Hs, Ws, inv, t, vt);
    lse[p] = l;
    float loss = 0.f;
    if (t != ignore) {
      loss = l - vt;
      if (weights) loss *= weights[p];
    }
    pixel_loss[p] = loss;
  }
}

__global__ void dl_init_kernel(DlState* __restrict__ st, unsigned k) {
  if (threadIdx.x == 0) { st->prefix = 0u; st->need = k; st->ties = 0u; st->pad = 0u; }
}

// digit histogram of the chunk's elements that match the digits chosen so far
__global__ __launch_bounds__(DL_THREADS) void dl_hist_kernel(const float* __restrict__ pixel_loss, long npix, long chunk,
                                                             const DlState* __restrict__ st, int shift,
                                                             unsigned* __restrict__ hist) {
  __shared__ unsigned h[DL_THREADS / 64][DL_BINS];
  const int t = threadIdx.x, wv = t >> 6;
  for (int i = t; i < (DL_THREADS / 64) * DL_BINS; i += DL_THREADS) (&h[0][0])[i] = 0u;
  __syncthreads();
  const unsigned prefix = st->prefix;
  const int above = shift + 8;     // bits above this digit must equal the prefix's
  const long p0 = (long)blockIdx.x * chunk, p1 = p0 + chunk < npix ? p0 + chunk : npix;
  for (long p = p0 + t; p < p1; p += DL_THREADS) {
    const unsigned key = ordered_bits(pixel_loss[p]);
    const bool match = above >= 32 || (key >> above) == (prefix >> above);
    if (match) atomicAdd(&h[wv][(key >> shift) & (DL_BINS - 1)], 1u);
  }
  __syncthreads();
  for (int d = t; d < DL_BINS; d += DL_THREADS) {
    unsigned s = 0u;
#pragma unroll
    for (int w = 0; w < DL_THREADS / 64; ++w) s += h[w][d];
    hist[(size_t)blockIdx.x * DL_BINS + d] = s;
  }
}

// one workgroup of DL_BINS x DL_SEL_SLICES threads: totals per bin (slice j adds workgroups j, j + DL_SEL_SLICES, ...;
// integer sums, any order gives the same), then the bin from the top in which the need-th element lies
__global__ __launch_bounds__(DL_BINS * DL_SEL_SLICES) void dl_select_kernel(const unsigned* __restrict__ hist, int wgs,
                                                                            int shift, DlState* __restrict__ st) {
  __shared__ unsigned tot[DL_SEL_SLICES][DL_BINS];
  const int d = threadIdx.x % DL_BINS, j = threadIdx.x / DL_BINS;
  unsigned s = 0u;
  for (int b = j; b < wgs; b += DL_SEL_SLICES) s += hist[(size_t)b * DL_BINS + d];
  tot[j][d] = s;
  __syncthreads();
  if (j == 0) {
    for (int jj = 1; jj < DL_SEL_SLICES; ++jj) s += tot[jj][d];
    tot[0][d] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned need = st->need, abovec = 0u;
    int bin = 0;
    for (int i = DL_BINS - 1; i >= 0; --i) {
      if (abovec + tot[0][i] >= need) { bin = i; break; }
      abovec += tot[0][i];
    }
    st->prefix |= (unsigned)bin << shift;
    st->need = need - abovec;
    st->ties = tot[0][bin];
  }
}

// per workgroup: the fp64 sum of the chunk's losses above the cut, and the number of its elements equal to the cut
__global__ __launch_bounds__(DL_THREADS) void dl_sum_kernel(const float* __restrict__ pixel_loss, long npix, long chunk,
                                                            const DlState* __restrict__ st, double* __restrict__ sums,
                                                            unsigned* __restrict__ tie_count) {
  __shared__ double sd[DL_THREADS];
  __shared__ unsigned sc[DL_THREADS];
  const int t = threadIdx.x;
  const unsigned cut = st->prefix;
  const long p0 = (long)blockIdx.x * chunk, p1 = p0 + chunk < npix ? p0 + chunk : npix;
  double s = 0.0;
  unsigned c = 0u;
  for (long p = p0 + t; p < p1; p += DL_THREADS) {
    const float l = pixel_loss[p];
    const unsigned key = ordered_bits(l);
    if (key > cut) s += (double)l;
    c += key == cut ? 1u : 0u;
  }
  sd[t] = s; sc[t] = c;
  __syncthreads();
  for (int o = DL_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) { sd[t] += sd[t + o]; sc[t] += sc[t + o]; }
    __syncthreads();
  }
  if (t == 0) { sums[blockIdx.x] = sd[0]; tie_count[blockIdx.x] = sc[0]; }
}

// the cut as the float it was (every NaN key is one NaN)
__device__ __forceinline__ float dl_cut_value(unsigned cut) {
  return cut == 0xffffffffu ? __uint_as_float(0x7fc00000u) : float_from_order_bits(cut);
}

// out[0] = (sum above the cut + need * cut) / k, out[1] = the cut; tie_base = exclusive scan of tie_count in
// workgroup order.  One workgroup of DL_THREADS: thread t owns the consecutive workgroups [t * per, (t + 1) * per), the
// threads' partial sums are added in thread order (a fixed order).
__global__ __launch_bounds__(DL_THREADS) void dl_finish_kernel(const double* __restrict__ sums,
                                                               const unsigned* __restrict__ tie_count, int wgs,
                                                               const DlState* __restrict__ st, unsigned k,
                                                               unsigned* __restrict__ tie_base, float* __restrict__ out) {
  __shared__ double sd[DL_THREADS];
  __shared__ unsigned sc[DL_THREADS];
  const int t = threadIdx.x, per = (wgs + DL_THREADS - 1) / DL_THREADS;
  const int b0 = t * per, b1 = min(wgs, b0 + per);
  double s = 0.0;
  unsigned c = 0u;
  for (int b = b0; b < b1; ++b) { s += sums[b]; c += tie_count[b]; }
  sd[t] = s; sc[t] = c;
  __syncthreads();
  if (t == 0) {
    double total = 0.0;
    unsigned base = 0u;
    for (int i = 0; i < DL_THREADS; ++i) {
      total += sd[i];
      const unsigned n = sc[i];
      sc[i] = base;
      base += n;
    }
    const float cut = dl_cut_value(st->prefix);
    out[0] = (float)((total + (double)st->need * (double)cut) / (double)k);
    out[1] = cut;
  }
  __syncthreads();
  unsigned base = sc[t];
  for (int b = b0; b < b1; ++b) {
    tie_base[b] = base;
    base += tie_count[b];
  }
}

// coef[p] = selected ? weight / k : 0; selected = above the cut, or equal to it and among the first `need` such pixels
// in flat order.  Ignored pixels get 0: they have no gradient.
__global__ __launch_bounds__(DL_THREADS) void dl_coef_kernel(const float* __restrict__ pixel_loss,
                                                             const long* __restrict__ target,
                                                             const float* __restrict__ weights, long npix, long chunk,
                                                             const DlState* __restrict__ st,
                                                             const unsigned* __restrict__ tie_base, float inv_k,
                                                             long ignore, float* __restrict__ coef) {
  __shared__ int wave_count[DL_THREADS / 64];
  const int t = threadIdx.x;
  const unsigned cut = st->prefix, need = st->need;
  unsigned base = tie_base[blockIdx.x];
  const long p0 = (long)blockIdx.x * chunk, p1 = p0 + chunk < npix ? p0 + chunk : npix;
  for (long q = p0; q < p1; q += DL_THREADS) {     // (uniform trip count: the compaction has barriers)
    const long p = q + t;
    const bool in = p < p1;
    const unsigned key = in ? ordered_bits(pixel_loss[p]) : 0u;
    const bool tie = in && key == cut;
    int total;
    const int slot = compact_wg<DL_THREADS / 64>(tie, wave_count, total);
    if (in) {
      const bool sel = key > cut || (tie && base + (unsigned)slot < need);
      float c = 0.f;
      if (sel && target[p] != ignore) c = weights ? weights[p] * inv_k : inv_k;
      coef[p] = c;
    }
    base += (unsigned)total;
  }
}

__global__ __launch_bounds__(256) void dl_bwd_kernel(const float* __restrict__ z, int ldc, int C,
                                                     const long* __restrict__ target, const float* __restrict__ lse,
                                                     const float* __restrict__ coef, const float* __restrict__ upstream,
                                                     float* __restrict__ dz, int N, int Hs, int Ws, int S, long ignore) {
  const int j = threadIdx.x & 15;
  const long nsrc = (long)N * Hs * Ws;
  const float inv = 1.f / (float)S;
  const float k = upstream ? *upstream : 1.f;
  const bool live = 4 * j < ldc;
  const int c0 = 4 * j;
  for (long p = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 4; p < nsrc; p += ((long)gridDim.x * blockDim.x) >> 4) {
    if (!live) continue;
    const int w = (int)(p % Ws);
    const long q = p / Ws;
    const int h = (int)(q % Hs), n = (int)(q / Hs);
    float acc[4];
    ce_gather_source<true>(z, ldc, C, target, lse, coef, n, h, w, c0, Hs, Ws, S, inv, ignore, acc);
    *reinterpret_cast<float4*>(dz + (size_t)p * ldc + c0) =
        make_float4(c0 + 0 < C ? acc[0] * k : 0.f, c0 + 1 < C ? acc[1] * k : 0.f, c0 + 2 < C ? acc[2] * k : 0.f,
                    c0 + 3 < C ? acc[3] * k : 0.f);
  }
}

int dl_check(int N, int Hs, int Ws, int S, int C, int ld, const char* what) {
  JTSM_REQUIRE(N >= 0 && Hs > 0 && Ws > 0 && S > 0 && C > 0 && C <= 64 && ld >= C && ld <= 64 && ld % 4 == 0,
               "%s: need C <= ld <= 64 and ld %% 4 == 0 (C=%d ld=%d)", what, C, ld);
  JTSM_REQUIRE((long)N * Hs * S * Ws * S < (1L << 31), "%s: fewer than 2^31 output pixels", what);
  return JTSM_OK;
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" {

size_t jtsm_deeplab_ce_workspace_bytes(void) { return dl_ws_bytes(); }

int jtsm_deeplab_ce_forward_f32(const float* logits, int ld, int C, const int64_t* target, const float* weights, long k,
                                float* lse, float* pixel_loss, float* coef, float* out, void* workspace, int N, int Hs,
                                int Ws, int S, long ignore_index, void* stream) {
  int rc = dl_check(N, Hs, Ws, S, C, ld, "deeplab_ce");
  if (rc) return rc;
  const long npix = (long)N * Hs * S * Ws * S;
  JTSM_REQUIRE(npix > 0 && k >= 1 && k <= npix, "deeplab_ce: need 1 <= k <= pixels (k=%ld, pixels=%ld)", k, npix);
  JTSM_REQUIRE(logits && target && lse && pixel_loss && coef && out && workspace, "deeplab_ce: null pointer");
  JTSM_REQUIRE(((uintptr_t)logits & 15) == 0, "deeplab_ce: logits must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const DlWs W = dl_carve(workspace);
  const DlChunks ch = dl_chunks(npix);
  const int blocks = (int)((npix + DL_THREADS - 1) / DL_THREADS < 2048 ? (npix + DL_THREADS - 1) / DL_THREADS : 2048);
  hipLaunchKernelGGL(dl_fwd_kernel, dim3(blocks), dim3(DL_THREADS), 0, st, logits, ld, C, (const long*)target, weights,
                     lse, pixel_loss, N, Hs, Ws, S, ignore_index);
  hipLaunchKernelGGL(dl_init_kernel, dim3(1), dim3(64), 0, st, W.st, (unsigned)k);
  for (int shift = 24; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(dl_hist_kernel, dim3(ch.wgs), dim3(DL_THREADS), 0, st, pixel_loss, npix, ch.chunk, W.st, shift,
                       W.hist);
    hipLaunchKernelGGL(dl_select_kernel, dim3(1), dim3(DL_BINS * DL_SEL_SLICES), 0, st, W.hist, ch.wgs, shift, W.st);
  }
  hipLaunchKernelGGL(dl_sum_kernel, dim3(ch.wgs), dim3(DL_THREADS), 0, st, pixel_loss, npix, ch.chunk, W.st, W.sums,
                     W.tie_count);
  hipLaunchKernelGGL(dl_finish_kernel, dim3(1), dim3(DL_THREADS), 0, st, W.sums, W.tie_count, ch.wgs, W.st, (unsigned)k,
                     W.tie_base, out);
  hipLaunchKernelGGL(dl_coef_kernel, dim3(ch.wgs), dim3(DL_THREADS), 0, st, pixel_loss, (const long*)target, weights,
                     npix, ch.chunk, W.st, W.tie_base, (float)(1.0 / (double)k), ignore_index, coef);
  JTSM_CHECK_LAUNCH("deeplab_ce forward");
  return JTSM_OK;
}

int jtsm_deeplab_ce_backward_f32(const float* logits, int ld, int C, const int64_t* target, const float* lse,
                                 const float* coef, const float* upstream, float* dlogits, int N, int Hs, int Ws, int S,
                                 long ignore_index, void* stream) {
  int rc = dl_check(N, Hs, Ws, S, C, ld, "deeplab_ce backward");
  if (rc) return rc;
  if (N == 0) return JTSM_OK;
  JTSM_REQUIRE(logits && target && lse && coef && dlogits, "deeplab_ce backward: null pointer");
  JTSM_REQUIRE(((uintptr_t)logits & 15) == 0 && ((uintptr_t)dlogits & 15) == 0,
               "deeplab_ce backward: logits and dlogits must be 16-byte aligned");
  const long nsrc = (long)N * Hs * Ws;
  const int blocks = (int)((nsrc + 15) / 16 < 16384 ? (nsrc + 15) / 16 : 16384);
  hipLaunchKernelGGL(dl_bwd_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), logits, ld, C, (const long*)target,
                     lse, coef, upstream, dlogits, N, Hs, Ws, S, ignore_index);
  JTSM_CHECK_LAUNCH("deeplab_ce backward");
  return JTSM_OK;
}

}  // extern "C"
