// Keypoint R-CNN on the device: heatmap targets, the spatial soft-max cross-entropy each way, the
// heatmap decode and the tail of the keypoint head (pixel shuffle of the 4x4 / stride-2 transposed convolution written
// as a 3x3 convolution, plus the x2 bilinear up-sampling).  Logits are plain contiguous (R, K, S, S): one (roi, keypoint)
// map is one row of S * S floats.  Built with -ffp-contract=off: the target cells and the decoded coordinates are the
// reference's fp32 expressions, every product and sum rounded.  No float atomics: every reduction has a fixed order.
#include "bilinear_ce.h"
#include "common.h"
#include "reduce.h"
#include "workspace.h"

namespace jtsm {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxSide = 64;                          // S <= 64: a row is at most 4096 floats, 16 per thread
constexpr int kPerThread = kMaxSide * kMaxSide / kThreads;
constexpr int kMaxOut = 16384;                        // decode: a box side is walked up to this many pixels

// (workgroup reductions in a fixed order — wg_reduce: reduce.h)

// ---- a. targets ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void targets_kernel(const float* __restrict__ kp, const float* __restrict__ rois,
                                                           int N, int K, int S, int* __restrict__ targets,
                                                           unsigned char* __restrict__ valid) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (long)N * K) return;
  const int n = (int)(i / K);
  const float x1 = rois[4 * n], y1 = rois[4 * n + 1], x2 = rois[4 * n + 2], y2 = rois[4 * n + 3];
  const float fs = (float)S;
  // the reference's `heatmap_size / (x2 - x1)` is torch's Tensor.__rtruediv__: reciprocal() * heatmap_size, rounded twice
  const float scale_x = (1.f / (x2 - x1)) * fs, scale_y = (1.f / (y2 - y1)) * fs;
  const float x = kp[3 * i], y = kp[3 * i + 1], v = kp[3 * i + 2];
  float cx = floorf((x - x1) * scale_x), cy = floorf((y - y1) * scale_y);
  if (x == x2) cx = fs - 1.f;
  if (y == y2) cy = fs - 1.f;
  // (a NaN or an infinite cell fails these comparisons, as the reference's cast to int64 puts it below zero)
  const bool ok = cx >= 0.f && cy >= 0.f && cx < fs && cy < fs && v > 0.f;
  targets[i] = ok ? (int)cy * S + (int)cx : 0;
  valid[i] = ok ? 1 : 0;
}

// ---- b. loss ------------------------------------------------------------------------------------------------------
// workspace: lse[rows] | row_loss[rows] | denom (1 float)
__global__ __launch_bounds__(kThreads) void loss_rows_kernel(const float* __restrict__ logits,
                                                             const int* __restrict__ targets,
                                                             const unsigned char* __restrict__ valid, int L,
                                                             float* __restrict__ lse, float* __restrict__ row_loss) {
  __shared__ float part[kWaves];
  const long row = blockIdx.x;
  const float* __restrict__ x = logits + row * L;
  float v[kPerThread];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const int e = threadIdx.x + j * kThreads;
    v[j] = e < L ? x[e] : -INFINITY;
    m = fmaxf(m, v[j]);
  }
  m = wg_reduce<kWaves>(m, Max(), part);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const int e = threadIdx.x + j * kThreads;
    if (e < L) s += expf(v[j] - m);
  }
  s = wg_reduce<kWaves>(s, Add(), part);
  if (threadIdx.x == 0) {
    const float l = m + logf(s);
    lse[row] = l;
    row_loss[row] = valid[row] ? l - x[min(max(targets[row], 0), L - 1)] : 0.f;
  }
}

__global__ __launch_bounds__(kThreads) void loss_total_kernel(const float* __restrict__ row_loss,
                                                              const unsigned char* __restrict__ valid, long rows,
                                                              float normalizer, float* __restrict__ loss,
                                                              float* __restrict__ denom) {
  __shared__ float part[kWaves];
  float s = 0.f, c = 0.f;
  for (long r = threadIdx.x; r < rows; r += kThreads) {
    s += row_loss[r];
    c += valid[r] ? 1.f : 0.f;
  }
  s = wg_reduce<kWaves>(s, Add(), part);
  c = wg_reduce<kWaves>(c, Add(), part);     // (a count: exact in fp32 up to 2^24 rows)
  if (threadIdx.x == 0) {
    const float d = normalizer > 0.f ? normalizer : (c > 0.f ? c : 1.f);
    *denom = d;
    *loss = c > 0.f ? s / d : 0.f;
  }
}

__global__ __launch_bounds__(kThreads) void loss_backward_kernel(const float* __restrict__ logits,
                                                                 const int* __restrict__ targets,
                                                                 const unsigned char* __restrict__ valid, int L,
                                                                 const float* __restrict__ lse,
                                                                 const float* __restrict__ denom,
                                                                 const float* __restrict__ g, float* __restrict__ dx) {
  const long row = blockIdx.x;
  float* __restrict__ out = dx + row * L;
  if (!valid[row]) {
    for (int e = threadIdx.x; e < L; e += kThreads) out[e] = 0.f;
    return;
  }
  const float* __restrict__ x = logits + row * L;
  const float l = lse[row], scale = *g / *denom;
  const int t = targets[row];
  for (int e = threadIdx.x; e < L; e += kThreads) out[e] = (expf(x[e] - l) - (e == t ? 1.f : 0.f)) * scale;
}

// ---- c. decode ----------------------------------------------------------------------------------------------------
// F.interpolate(mode="bicubic", align_corners=False): A = -0.75, taps floor(src) - 1 .. + 2 clamped to the border.
__device__ __forceinline__ void cubic_coefficients(float t, float c[4]) {
  const float A = -0.75f;
  const float a = t + 1.f, b = 1.f - t, d = b + 1.f;
  c[0] = ((A * a - 5.f * A) * a + 8.f * A) * a - 4.f * A;
  c[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  c[2] = ((A + 2.f) * b - (A + 3.f)) * b * b + 1.f;
  c[3] = ((A * d - 5.f * A) * d + 8.f * A) * d - 4.f * A;
}

__global__ __launch_bounds__(kThreads) void decode_kernel(const float* __restrict__ maps, const float* __restrict__ rois,
                                                          int K, int S, float* __restrict__ out) {
  __shared__ float tile[kMaxSide * kMaxSide];
  __shared__ float part[kWaves];
  __shared__ float best_v[kWaves];
  __shared__ unsigned best_i[kWaves];
  const long row = blockIdx.x;
  const int r = (int)(row / K), L = S * S;
  const float* __restrict__ src = maps + row * L;
  for (int e = threadIdx.x; e < L; e += kThreads) tile[e] = src[e];
  const float x1 = rois[4 * r], y1 = rois[4 * r + 1];
  const float w = fmaxf(rois[4 * r + 2] - x1, 1.f), h = fmaxf(rois[4 * r + 3] - y1, 1.f);
  const int ow = (int)fminf(ceilf(w), (float)kMaxOut), oh = (int)fminf(ceilf(h), (float)kMaxOut);
  const float sx = (float)S / (float)ow, sy = (float)S / (float)oh;
  __syncthreads();
  const unsigned total = (unsigned)ow * (unsigned)oh;
  float bv = -INFINITY;
  unsigned bi = 0xffffffffu;
  for (unsigned p = threadIdx.x; p < total; p += kThreads) {
    const unsigned oy = p / (unsigned)ow, ox = p - oy * (unsigned)ow;
    const float rx = sx * ((float)ox + 0.5f) - 0.5f, ry = sy * ((float)oy + 0.5f) - 0.5f;
    const float fx = floorf(rx), fy = floorf(ry);
    float cx[4], cy[4];
    cubic_coefficients(rx - fx, cx);
    cubic_coefficients(ry - fy, cy);
    const int ix = (int)fx, iy = (int)fy;
    int xs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xs[j] = min(max(ix - 1 + j, 0), S - 1);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float* __restrict__ line = tile + min(max(iy - 1 + i, 0), S - 1) * S;
      const float hsum = line[xs[0]] * cx[0] + line[xs[1]] * cx[1] + line[xs[2]] * cx[2] + line[xs[3]] * cx[3];
      acc += hsum * cy[i];
    }
    if (acc > bv) { bv = acc; bi = p; }      // p grows: a tie keeps the lower index
  }
  // arg-max across the workgroup, ties to the lowest flat index: wg_arg_best's rule (reduce.h), written out — through
  // wg_arg_best the decode measured 1-2 % slower
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const unsigned oi = __shfl_xor(bi, o);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if ((threadIdx.x & 63) == 0) { best_v[threadIdx.x >> 6] = bv; best_i[threadIdx.x >> 6] = bi; }
  __syncthreads();
  bv = best_v[0];
  bi = best_i[0];
#pragma unroll
  for (int k = 1; k < kWaves; ++k)
    if (best_v[k] > bv || (best_v[k] == bv && best_i[k] < bi)) { bv = best_v[k]; bi = best_i[k]; }
  if (bi == 0xffffffffu) bi = 0;             // (a map of NaN only)
  float s = 0.f;
  for (int e = threadIdx.x; e < L; e += kThreads) s += expf(tile[e] - bv);
  s = wg_reduce<kWaves>(s, Add(), part);
  if (threadIdx.x == 0) {
    const unsigned yi = (unsigned)bi / (unsigned)ow, xi = (unsigned)bi - yi * (unsigned)ow;
    const float corr_x = w / (float)ow, corr_y = h / (float)oh;
    out[4 * row] = ((float)xi + 0.5f) * corr_x + x1;
    out[4 * row + 1] = ((float)yi + 0.5f) * corr_y + y1;
    out[4 * row + 2] = bv;
    out[4 * row + 3] = 1.f / s;
  }
}

// ---- d. pixel shuffle + bilinear x2 -------------------------------------------------------------------------------
// F.interpolate(scale_factor=2, mode="bilinear", align_corners=False): lerp_scale at 1 / 2 along each axis
// z (R, H, W, Cp) channels-last, channel (py * 2 + px) * K + k holds pixel (2 i + py, 2 j + px) of keypoint k
__device__ __forceinline__ float shuffled(const float* __restrict__ z, int H, int W, int Cp, int K, int k, int a,
                                          int b) {
  return z[((long)(a >> 1) * W + (b >> 1)) * Cp + ((a & 1) * 2 + (b & 1)) * K + k];
}

__global__ __launch_bounds__(kThreads) void upsample_forward_kernel(const float* __restrict__ z, long total, int K,
                                                                    int H, int W, int Cp, float* __restrict__ out) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int OW = 4 * W, OH = 4 * H;
  const int X = (int)(i % OW), Y = (int)((i / OW) % OH), k = (int)((i / ((long)OW * OH)) % K);
  const long r = i / ((long)OW * OH * K);
  const float* __restrict__ zr = z + r * (long)H * W * Cp;
  const Lerp a = lerp_scale(Y, 2 * H, 0.5f), b = lerp_scale(X, 2 * W, 0.5f);
  out[i] = blend(a, b, shuffled(zr, H, W, Cp, K, k, a.i0, b.i0), shuffled(zr, H, W, Cp, K, k, a.i0, b.i1),
                 shuffled(zr, H, W, Cp, K, k, a.i1, b.i0), shuffled(zr, H, W, Cp, K, k, a.i1, b.i1));
}

// The adjoint as a gather: element (r, i, j, c) of dz collects every output pixel whose taps name its shuffled pixel.
__global__ __launch_bounds__(kThreads) void upsample_backward_kernel(const float* __restrict__ g, long total, int K,
                                                                     int H, int W, int Cp, float* __restrict__ dz) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % Cp), j = (int)((i / Cp) % W), ii = (int)((i / ((long)Cp * W)) % H);
  const long r = i / ((long)Cp * W * H);
  if (c >= 4 * K) { dz[i] = 0.f; return; }
  const int par = c / K, k = c - par * K;
  const int a = 2 * ii + (par >> 1), b = 2 * j + (par & 1);
  const int OW = 4 * W, OH = 4 * H;
  const float* __restrict__ gr = g + (r * K + k) * (long)OH * OW;
  float acc = 0.f;
  for (int Y = max(2 * a - 1, 0); Y <= min(2 * a + 2, OH - 1); ++Y) {
    const Lerp ty = lerp_scale(Y, 2 * H, 0.5f);
    const float wy = (ty.i0 == a ? ty.l0 : 0.f) + (ty.i1 == a ? ty.l1 : 0.f);
    if (wy == 0.f) continue;
    float line = 0.f;
    for (int X = max(2 * b - 1, 0); X <= min(2 * b + 2, OW - 1); ++X) {
      const Lerp tx = lerp_scale(X, 2 * W, 0.5f);
      const float wx = (tx.i0 == b ? tx.l0 : 0.f) + (tx.i1 == b ? tx.l1 : 0.f);
      line += wx * gr[(long)Y * OW + X];
    }
    acc += wy * line;
  }
  dz[i] = acc;
}

// lse[rows] | row_loss[rows] | the denominator: one float, the last 256 bytes of the published size
struct LossWs { float* lse; float* row_loss; float* denom; };
LossWs carve_loss(Arena& a, size_t rows) {
  LossWs w;
  w.lse = a.take<float>(rows);
  w.row_loss = a.take<float>(rows);
  w.denom = a.take<float>(1);
  return w;
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" {

int jtsm_keypoint_targets_f32(const float* keypoints, const float* rois, int N, int K, int S, int32_t* targets,
                              uint8_t* valid, void* stream) {
  JTSM_REQUIRE(N >= 0 && K >= 1 && S >= 1 && (long)S * S < (1L << 31), "keypoint_targets: N=%d K=%d S=%d", N, K, S);
  if (N == 0) return JTSM_OK;
  JTSM_REQUIRE(keypoints && rois && targets && valid, "keypoint_targets: null pointer");
  hipLaunchKernelGGL(targets_kernel, dim3(ceil_div((long)N * K, kThreads)), dim3(kThreads), 0, as_stream(stream),
                     keypoints, rois, N, K, S, targets, valid);
  JTSM_CHECK_LAUNCH("keypoint_targets");
  return JTSM_OK;
}

size_t jtsm_keypoint_loss_workspace_bytes(int N, int K) {
  const size_t rows = (size_t)(N > 0 ? N : 0) * (size_t)(K > 0 ? K : 0);
  Arena a{nullptr};
  carve_loss(a, rows);
  return a.off;
}

int jtsm_keypoint_loss_forward_f32(const float* logits, const int32_t* targets, const uint8_t* valid, int N, int K,
                                   int S, float normalizer, float* loss, void* workspace, void* stream) {
  JTSM_REQUIRE(N >= 0 && K >= 1 && S >= 1 && S <= kMaxSide, "keypoint_loss: N=%d K=%d S=%d (S <= %d)", N, K, S, kMaxSide);
  JTSM_REQUIRE(loss && workspace, "keypoint_loss: null pointer");
  const long rows = (long)N * K;
  JTSM_REQUIRE(rows < (1L << 24), "keypoint_loss: %ld rows (the valid count is kept in fp32)", rows);
  Arena arena{static_cast<char*>(workspace)};
  const LossWs w = carve_loss(arena, (size_t)rows);
  if (rows) {
    JTSM_REQUIRE(logits && targets && valid, "keypoint_loss: null pointer");
    hipLaunchKernelGGL(loss_rows_kernel, dim3((unsigned)rows), dim3(kThreads), 0, as_stream(stream), logits, targets,
                       valid, S * S, w.lse, w.row_loss);
    JTSM_CHECK_LAUNCH("keypoint_loss rows");
  }
  hipLaunchKernelGGL(loss_total_kernel, dim3(1), dim3(kThreads), 0, as_stream(stream), w.row_loss, valid, rows,
                     normalizer, loss, w.denom);
  JTSM_CHECK_LAUNCH("keypoint_loss total");
  return JTSM_OK;
}

int jtsm_keypoint_loss_backward_f32(const float* logits, const int32_t* targets, const uint8_t* valid, int N, int K,
                                    int S, const float* grad_loss, const void* workspace, float* grad_logits,
                                    void* stream) {
  JTSM_REQUIRE(N >= 0 && K >= 1 && S >= 1 && S <= kMaxSide, "keypoint_loss: N=%d K=%d S=%d (S <= %d)", N, K, S, kMaxSide);
  const long rows = (long)N * K;
  if (rows == 0) return JTSM_OK;
  JTSM_REQUIRE(logits && targets && valid && grad_loss && workspace && grad_logits, "keypoint_loss: null pointer");
  Arena arena{static_cast<char*>(const_cast<void*>(workspace))};
  const LossWs w = carve_loss(arena, (size_t)rows);
  hipLaunchKernelGGL(loss_backward_kernel, dim3((unsigned)rows), dim3(kThreads), 0, as_stream(stream), logits, targets,
                     valid, S * S, w.lse, w.denom, grad_loss, grad_logits);
  JTSM_CHECK_LAUNCH("keypoint_loss backward");
  return JTSM_OK;
}

int jtsm_keypoint_decode_f32(const float* maps, const float* rois, int R, int K, int S, float* out, void* stream) {
  JTSM_REQUIRE(R >= 0 && K >= 1 && S >= 1 && S <= kMaxSide, "keypoint_decode: R=%d K=%d S=%d (S <= %d)", R, K, S, kMaxSide);
  if (R == 0) return JTSM_OK;
  JTSM_REQUIRE(maps && rois && out, "keypoint_decode: null pointer");
  JTSM_REQUIRE((long)R * K < (1L << 31), "keypoint_decode: %ld maps", (long)R * K);
  hipLaunchKernelGGL(decode_kernel, dim3((unsigned)((long)R * K)), dim3(kThreads), 0, as_stream(stream), maps, rois, K,
                     S, out);
  JTSM_CHECK_LAUNCH("keypoint_decode");
  return JTSM_OK;
}

int jtsm_keypoint_upsample_forward_f32(const float* z, int R, int K, int H, int W, int Cp, float* logits,
                                       void* stream) {
  JTSM_REQUIRE(R >= 0 && K >= 1 && H >= 1 && W >= 1 && Cp >= 4 * K, "keypoint_upsample: R=%d K=%d H=%d W=%d Cp=%d", R,
               K, H, W, Cp);
  const long total = (long)R * K * 16 * H * W;
  if (total == 0) return JTSM_OK;
  JTSM_REQUIRE(z && logits, "keypoint_upsample: null pointer");
  JTSM_REQUIRE(total / kThreads < (1L << 31), "keypoint_upsample: %ld outputs", total);
  hipLaunchKernelGGL(upsample_forward_kernel, dim3(ceil_div(total, kThreads)), dim3(kThreads), 0, as_stream(stream), z,
                     total, K, H, W, Cp, logits);
  JTSM_CHECK_LAUNCH("keypoint_upsample forward");
  return JTSM_OK;
}

int jtsm_keypoint_upsample_backward_f32(const float* grad_logits, int R, int K, int H, int W, int Cp, float* grad_z,
                                        void* stream) {
  JTSM_REQUIRE(R >= 0 && K >= 1 && H >= 1 && W >= 1 && Cp >= 4 * K, "keypoint_upsample: R=%d K=%d H=%d W=%d Cp=%d", R,
               K, H, W, Cp);
  const long total = (long)R * H * W * Cp;
  if (total == 0) return JTSM_OK;
  JTSM_REQUIRE(grad_logits && grad_z, "keypoint_upsample: null pointer");
  JTSM_REQUIRE(total / kThreads < (1L << 31), "keypoint_upsample: %ld elements", total);
  hipLaunchKernelGGL(upsample_backward_kernel, dim3(ceil_div(total, kThreads)), dim3(kThreads), 0, as_stream(stream),
                     grad_logits, total, K, H, W, Cp, grad_z);
  JTSM_CHECK_LAUNCH("keypoint_upsample backward");
  return JTSM_OK;
}

}  // extern "C"
