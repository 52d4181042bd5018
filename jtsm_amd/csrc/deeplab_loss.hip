// DeepLabCE, the hard-pixel-mining cross-entropy (projects/DeepLab/deeplab/loss.py:6-40), fused with the bilinear xS
// up-sampling that precedes it (projects/DeepLab/deeplab/semantic_seg.py: F.interpolate(..., scale_factor=
// common_stride, mode="bilinear", align_corners=False) in DeepLabV3PlusHead.losses / DeepLabV3Head.losses).  The
// reference materialises the up-sampled logits, the per-pixel losses, and sorts them (torch.topk); here
//   forward   one thread per output pixel interpolates its logits on the fly (bilinear_ce.h, the code of
//             semseg_ops.hip) and writes the log-sum-exp and the per-pixel loss, 4 B each (0 where the target is
//             ignored, times `weights` where given);
//   select    the k-th largest loss is found by the chunked radix select of select.h (its header states the key order:
//             -0 = +0, every NaN on top, so a NaN loss is among the chosen and the result is NaN, as with torch.topk).
//             Nothing is read back; the workspace is the histograms and a few words per workgroup, whatever the
//             number of pixels;
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
#include "select.h"
#include "workspace.h"

namespace jtsm {
namespace {

constexpr int DL_THREADS = kChunkThreads;     // the chunked passes (select.h) and the forward alike

struct DlWs {
  unsigned* hist;       // [kMaxChunkWgs][kSelectBins]
  SelectState* st;
  unsigned* tie_count;  // [kMaxChunkWgs]
  unsigned* tie_base;   // [kMaxChunkWgs]
  double* sums;         // [kMaxChunkWgs]
};
DlWs carve(Arena& a) {
  DlWs W;
  W.hist = a.take<unsigned>(kMaxChunkWgs * kSelectBins);
  W.st = a.take<SelectState>(1);
  W.tie_count = a.take<unsigned>(kMaxChunkWgs);
  W.tie_base = a.take<unsigned>(kMaxChunkWgs);
  W.sums = a.take<double>(kMaxChunkWgs);
  return W;
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

// per workgroup: the fp64 sum of the chunk's losses above the cut, and the number of its elements equal to the cut
__global__ __launch_bounds__(DL_THREADS) void dl_sum_kernel(const float* __restrict__ pixel_loss, long npix, long chunk,
                                                            const SelectState* __restrict__ st,
                                                            double* __restrict__ sums, unsigned* __restrict__ tie_count) {
  __shared__ double sd[DL_THREADS];
  __shared__ unsigned sc[DL_THREADS];
  const unsigned cut = st->prefix;
  const ChunkSpan ch = chunk_of_wg(npix, chunk);
  double s = 0.0;
  unsigned c = 0u;
  for (long p = ch.p0 + threadIdx.x; p < ch.p1; p += DL_THREADS) {
    const float l = pixel_loss[p];
    const unsigned key = ordered_bits(l);
    if (key > cut) s += (double)l;
    c += key == cut ? 1u : 0u;
  }
  wg_tree_sum<DL_THREADS>(s, sd, c, sc);
  if (threadIdx.x == 0) { sums[blockIdx.x] = s; tie_count[blockIdx.x] = c; }
}

// out[0] = (sum above the cut + need * cut) / k, out[1] = the cut; tie_base = the exclusive scan of tie_count in
// workgroup order.  Both from the fixed-order fold of reduce.h: it leaves in sc[t] the ties of the threads before t,
// from which thread t scans its own consecutive workgroups.
__global__ __launch_bounds__(DL_THREADS) void dl_finish_kernel(const double* __restrict__ sums,
                                                               const unsigned* __restrict__ tie_count, int wgs,
                                                               const SelectState* __restrict__ st, unsigned k,
                                                               unsigned* __restrict__ tie_base, float* __restrict__ out) {
  __shared__ double sd[DL_THREADS];
  __shared__ unsigned sc[DL_THREADS];
  double total;
  unsigned ties;
  fold_chunks<DL_THREADS>(sums, tie_count, 1, wgs, sd, sc, total, ties);
  if (threadIdx.x == 0) {
    const float cut = cut_value(st->prefix);
    out[0] = (float)((total + (double)st->need * (double)cut) / (double)k);
    out[1] = cut;
  }
  __syncthreads();
  const FoldSpan f = fold_span<DL_THREADS>(wgs);
  unsigned base = sc[threadIdx.x];
  for (int b = f.b0; b < f.b1; ++b) {
    tie_base[b] = base;
    base += tie_count[b];
  }
}

// coef[p] = selected ? weight / k : 0; selected = above the cut, or equal to it and among the first `need` such pixels
// in flat order.  Ignored pixels get 0: they have no gradient.
__global__ __launch_bounds__(DL_THREADS) void dl_coef_kernel(const float* __restrict__ pixel_loss,
                                                             const long* __restrict__ target,
                                                             const float* __restrict__ weights, long npix, long chunk,
                                                             const SelectState* __restrict__ st,
                                                             const unsigned* __restrict__ tie_base, float inv_k,
                                                             long ignore, float* __restrict__ coef) {
  __shared__ int wave_count[DL_THREADS / 64];
  const int t = threadIdx.x;
  const unsigned cut = st->prefix, need = st->need;
  unsigned base = tie_base[blockIdx.x];
  const ChunkSpan ch = chunk_of_wg(npix, chunk);
  for (long q = ch.p0; q < ch.p1; q += DL_THREADS) {     // (uniform trip count: the compaction has barriers)
    const long p = q + t;
    const bool in = p < ch.p1;
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

size_t jtsm_deeplab_ce_workspace_bytes(void) {
  Arena a{nullptr, false, 16};
  carve(a);
  return a.off + 16;
}

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
  Arena arena{static_cast<char*>(workspace), false, 16};
  const DlWs W = carve(arena);
  const Chunks ch = chunks_of(npix);
  const int blocks = (int)((npix + DL_THREADS - 1) / DL_THREADS < 2048 ? (npix + DL_THREADS - 1) / DL_THREADS : 2048);
  hipLaunchKernelGGL(dl_fwd_kernel, dim3(blocks), dim3(DL_THREADS), 0, st, logits, ld, C, (const long*)target, weights,
                     lse, pixel_loss, N, Hs, Ws, S, ignore_index);
  launch_select(pixel_loss, npix, ch, (unsigned)k, W.st, W.hist, st);
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
