// Trainable batch norm on channels-last fp32 maps: rows of C channels with a leading dimension (a [:, :C] slice of a
// wider map is fine).  Replaces torch.nn.BatchNorm2d / SyncBatchNorm / NaiveSyncBatchNorm behind a convolution
// (detectron2/layers/batch_norm.py:128-153, wrappers.py:79-82) in training mode; in evaluation mode no kernel of this
// file runs (layers/batch_norm.py: scale_bias() folds into the contraction's epilogue).
//
// Shape of the GroupNorm kernels of semseg_ops.hip: statistics, fold, apply.
//   statistics  every thread owns V channels (V = 4 as one float4 where C, the leading dimension and the pointer allow
//               it, else 1) and every TY-th row of its slab.  It sums (x - K) and (x - K)^2 with K = ITS FIRST VALUE,
//               so the sums are of the size of the spread, not of the mean: a map whose mean is large against its
//               spread keeps its variance (one-pass fp32 E[x^2] - E[x]^2 loses it).  The thread's (count, mean, M2)
//               and then the workgroup's are combined by the pairwise update (Chan et al.) in fp64, in a fixed tree.
//   fold        per channel, eight slices of the slabs' (count, mean, M2) combined in a fixed order, fp64.
//   apply       one pass, y = relu?((x - mean) * invstd * gamma + beta (+ residual)).
// No floating-point atomics anywhere: the same input gives the same bits.
//
// The backward is one reduction (sum dy, sum dy * xhat per channel, dy gated by y > 0 where the forward applied the
// ReLU: these are dbeta and dgamma) and one apply pass (dx, and d residual = the gated dy).
//
// Between statistics and apply, and between the backward's reduction and apply, the per-channel vectors are plain
// device arrays: a multi-process run all-reduces them there (layers/batch_norm.py: combine_statistics).
#include "common.h"
#include "workspace.h"

namespace jtsm {
namespace {

struct BnGeom {
  int V, cols, tx, ty, gx, slabs;
  long rps;   // rows per slab
};

inline BnGeom bn_geom(long R, int C, bool vec) {
  BnGeom g;
  g.V = vec ? 4 : 1;
  g.cols = C / g.V;
  g.tx = 1;
  while (g.tx < g.cols && g.tx < 64) g.tx <<= 1;
  g.ty = 256 / g.tx;
  g.gx = (g.cols + g.tx - 1) / g.tx;
  const long per = (long)g.ty * 16;                 // 16 rows per thread where the map has them
  long want = (R + per - 1) / per;
  const long cap = 2048 / g.gx > 1 ? 2048 / g.gx : 1;
  if (want > cap) want = cap;
  if (want < 1) want = 1;
  g.rps = (R + want - 1) / want;
  if (g.rps < 1) g.rps = 1;
  g.slabs = (int)((R + g.rps - 1) / g.rps);
  if (g.slabs < 1) g.slabs = 1;
  return g;
}

inline bool bn_vec_ok(int C, long ld, const void* a, const void* b = nullptr, const void* c = nullptr,
                      const void* d = nullptr) {
  auto al = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  return C % 4 == 0 && ld % 4 == 0 && al(a) && al(b) && al(c) && al(d);
}

template <int V> struct Vec;
template <> struct Vec<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
  __device__ __forceinline__ void store(float* p) const { *p = v[0]; }
};
template <> struct Vec<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

// (count, mean, M2) of a and b together, into a
__device__ __forceinline__ void chan_merge(double& na, double& ma, double& qa, double nb, double mb, double qb) {
  if (nb == 0.0) return;
  if (na == 0.0) { na = nb; ma = mb; qa = qb; return; }
  const double n = na + nb, d = mb - ma;
  ma += d * (nb / n);
  qa += qb + d * d * (na * nb / n);
  na = n;
}

// ---- forward statistics: part[slab][0][c] = mean, part[slab][1][c] = M2 of the slab's rows (their count follows from
// the geometry).  blockDim = (tx, ty), grid = (gx, slabs).
template <int V>
__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ x, long ld, long R, int C, long rps,
                                                       double* __restrict__ part) {
  __shared__ double sn[256], sm[256 * V], sq[256 * V];
  const int tx = threadIdx.x, ty = threadIdx.y, TX = blockDim.x, TY = blockDim.y;
  const int col = blockIdx.x * TX + tx, c0 = col * V;
  const bool live = c0 < C;
  const long r0 = (long)blockIdx.y * rps, r1 = r0 + rps < R ? r0 + rps : R;
  float K[V], s[V], q[V];
#pragma unroll
  for (int e = 0; e < V; ++e) { K[e] = 0.f; s[e] = 0.f; q[e] = 0.f; }
  int n = 0;
  if (live)
    for (long r = r0 + ty; r < r1; r += TY) {
      Vec<V> t;
      t.load(x + r * ld + c0);
      if (n == 0) {
#pragma unroll
        for (int e = 0; e < V; ++e) K[e] = t.v[e];
      }
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float d = t.v[e] - K[e];
        s[e] += d;
        q[e] += d * d;
      }
      ++n;
    }
  const int me = ty * TX + tx;
  sn[me] = (double)n;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const double sd = s[e], nd = n > 0 ? (double)n : 1.0;
    sm[me * V + e] = (double)K[e] + sd / nd;
    const double m2 = (double)q[e] - sd * sd / nd;
    sq[me * V + e] = m2 > 0.0 ? m2 : 0.0;
  }
  __syncthreads();
  for (int o = TY >> 1; o > 0; o >>= 1) {
    if (ty < o) {
      const int other = (ty + o) * TX + tx;
      double n_both = sn[me];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        n_both = sn[me];   // (the V channels of a thread share their counts)
        chan_merge(n_both, sm[me * V + e], sq[me * V + e], sn[other], sm[other * V + e], sq[other * V + e]);
      }
      sn[me] = n_both;
    }
    __syncthreads();
  }
  if (ty == 0 && live) {
    double* p = part + (size_t)blockIdx.y * 2 * C;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      p[c0 + e] = sm[me * V + e];
      p[C + c0 + e] = sq[me * V + e];
    }
  }
}

// invstd and the running statistics of one channel from (mean, M2) over `n` values, as torch.nn.BatchNorm2d forms them:
// the biased variance normalises, the unbiased one goes into running_var; `factor` is the momentum.
__device__ __forceinline__ void bn_finalize_one(int c, double mean, double m2, double n, float eps, float factor,
                                                float* __restrict__ invstd, float* __restrict__ running_mean,
                                                float* __restrict__ running_var) {
  double var = m2 / n;
  if (var < 0.0) var = 0.0;
  invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) running_mean[c] = (float)((1.0 - (double)factor) * (double)running_mean[c] + (double)factor * mean);
  if (running_var) {
    const double unbiased = m2 / (n - 1.0);
    running_var[c] = (float)((1.0 - (double)factor) * (double)running_var[c] + (double)factor * unbiased);
  }
}

// The slabs of a channel: 256 threads = FOLD_TC channels x FOLD_TS slices; slice j combines slabs j, j + FOLD_TS, ... in
// that order, then the slices are combined in slice order (a fixed order: the same bits on every run; one thread per
// channel over ~1000 slabs would be ~1000 dependent fp64 divisions, longer than the pass over the map).  With invstd
// given, also what bn_finalize_one writes (single-process form).
constexpr int FOLD_TC = 32, FOLD_TS = 8;
__global__ __launch_bounds__(256) void bn_fold_kernel(const double* __restrict__ part, long R, int C, long rps, int slabs,
                                                      float* __restrict__ mean, float* __restrict__ m2, float eps,
                                                      float factor, float* __restrict__ invstd,
                                                      float* __restrict__ running_mean, float* __restrict__ running_var) {
  __shared__ double sn[FOLD_TS][FOLD_TC], sm[FOLD_TS][FOLD_TC], sq[FOLD_TS][FOLD_TC];
  const int tc = threadIdx.x % FOLD_TC, j = threadIdx.x / FOLD_TC;
  const int c = blockIdx.x * FOLD_TC + tc;
  double n = 0.0, m = 0.0, q = 0.0;
  if (c < C)
    for (int s = j; s < slabs; s += FOLD_TS) {
      const long r0 = (long)s * rps, r1 = r0 + rps < R ? r0 + rps : R;
      chan_merge(n, m, q, (double)(r1 - r0), part[(size_t)s * 2 * C + c], part[(size_t)s * 2 * C + C + c]);
    }
  sn[j][tc] = n; sm[j][tc] = m; sq[j][tc] = q;
  __syncthreads();
  if (j != 0 || c >= C) return;
  for (int jj = 1; jj < FOLD_TS; ++jj) chan_merge(n, m, q, sn[jj][tc], sm[jj][tc], sq[jj][tc]);
  mean[c] = (float)m;
  m2[c] = (float)q;
  if (invstd) bn_finalize_one(c, m, q, n, eps, factor, invstd, running_mean, running_var);
}

__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ mean, const float* __restrict__ m2,
                                                          double n, int C, float eps, float factor,
                                                          float* __restrict__ invstd, float* __restrict__ running_mean,
                                                          float* __restrict__ running_var) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) bn_finalize_one(c, (double)mean[c], (double)m2[c], n, eps, factor, invstd, running_mean, running_var);
}

// y = relu?((x - mean) * invstd * gamma + beta (+ residual)); y and residual are dense rows of C
template <int V, bool RES>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, long ld,
                                                       const float* __restrict__ residual,
                                                       const float* __restrict__ mean, const float* __restrict__ invstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float* __restrict__ y, long R, int C, int relu) {
  const int c0 = (blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (c0 >= C) return;
  Vec<V> mu, rs, ga, be;
  mu.load(mean + c0); rs.load(invstd + c0); ga.load(gamma + c0); be.load(beta + c0);
  for (long r = (long)blockIdx.y * blockDim.y + threadIdx.y; r < R; r += (long)gridDim.y * blockDim.y) {
    Vec<V> t, o, rr;
    t.load(x + r * ld + c0);
    if (RES) rr.load(residual + r * C + c0);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float v = (t.v[e] - mu.v[e]) * rs.v[e] * ga.v[e] + be.v[e];
      if (RES) v += rr.v[e];
      o.v[e] = relu ? fmaxf(v, 0.f) : v;
    }
    o.store(y + r * C + c0);
  }
}

// ---- backward reduction: part[slab][0][c] = sum g, part[slab][1][c] = sum g * xhat, g = dy gated by y > 0
template <int V>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ x, long ld,
                                                            const float* __restrict__ dy, const float* __restrict__ y,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, long R, int C, long rps,
                                                            int relu, double* __restrict__ part) {
  __shared__ double sa[256 * V], sb[256 * V];
  const int tx = threadIdx.x, ty = threadIdx.y, TX = blockDim.x, TY = blockDim.y;
  const int c0 = (blockIdx.x * TX + tx) * V;
  const bool live = c0 < C;
  const long r0 = (long)blockIdx.y * rps, r1 = r0 + rps < R ? r0 + rps : R;
  float a[V], b[V];
#pragma unroll
  for (int e = 0; e < V; ++e) { a[e] = 0.f; b[e] = 0.f; }
  if (live) {
    Vec<V> mu, rs;
    mu.load(mean + c0); rs.load(invstd + c0);
    for (long r = r0 + ty; r < r1; r += TY) {
      Vec<V> t, d, o;
      t.load(x + r * ld + c0);
      d.load(dy + r * C + c0);
      if (relu) o.load(y + r * C + c0);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float g = (relu && !(o.v[e] > 0.f)) ? 0.f : d.v[e];
        a[e] += g;
        b[e] += g * ((t.v[e] - mu.v[e]) * rs.v[e]);
      }
    }
  }
  const int me = ty * TX + tx;
#pragma unroll
  for (int e = 0; e < V; ++e) { sa[me * V + e] = (double)a[e]; sb[me * V + e] = (double)b[e]; }
  __syncthreads();
  for (int o = TY >> 1; o > 0; o >>= 1) {
    if (ty < o) {
      const int other = (ty + o) * TX + tx;
#pragma unroll
      for (int e = 0; e < V; ++e) { sa[me * V + e] += sa[other * V + e]; sb[me * V + e] += sb[other * V + e]; }
    }
    __syncthreads();
  }
  if (ty == 0 && live) {
    double* p = part + (size_t)blockIdx.y * 2 * C;
#pragma unroll
    for (int e = 0; e < V; ++e) { p[c0 + e] = sa[me * V + e]; p[C + c0 + e] = sb[me * V + e]; }
  }
}

__global__ __launch_bounds__(256) void bn_bwd_fold_kernel(const double* __restrict__ part, int C, int slabs,
                                                          float* __restrict__ sum_dy, float* __restrict__ sum_dy_xhat) {
  __shared__ double sa[FOLD_TS][FOLD_TC], sb[FOLD_TS][FOLD_TC];     // (slices as in bn_fold_kernel)
  const int tc = threadIdx.x % FOLD_TC, j = threadIdx.x / FOLD_TC;
  const int c = blockIdx.x * FOLD_TC + tc;
  double a = 0.0, b = 0.0;
  if (c < C)
    for (int s = j; s < slabs; s += FOLD_TS) { a += part[(size_t)s * 2 * C + c]; b += part[(size_t)s * 2 * C + C + c]; }
  sa[j][tc] = a; sb[j][tc] = b;
  __syncthreads();
  if (j != 0 || c >= C) return;
  for (int jj = 1; jj < FOLD_TS; ++jj) { a += sa[jj][tc]; b += sb[jj][tc]; }
  sum_dy[c] = (float)a;
  sum_dy_xhat[c] = (float)b;
}

// dx = gamma * invstd * (g - sum_dy / n - xhat * sum_dy_xhat / n); d residual = g
template <int V, bool RES>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ x, long ld,
                                                           const float* __restrict__ dy, const float* __restrict__ y,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ invstd,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ sum_dy,
                                                           const float* __restrict__ sum_dy_xhat, float inv_n,
                                                           float* __restrict__ dx, float* __restrict__ dres, long R,
                                                           int C, int relu) {
  const int c0 = (blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (c0 >= C) return;
  Vec<V> mu, rs, ga, A, B;
  mu.load(mean + c0); rs.load(invstd + c0); ga.load(gamma + c0); A.load(sum_dy + c0); B.load(sum_dy_xhat + c0);
#pragma unroll
  for (int e = 0; e < V; ++e) { A.v[e] *= inv_n; B.v[e] *= inv_n; ga.v[e] *= rs.v[e]; }
  for (long r = (long)blockIdx.y * blockDim.y + threadIdx.y; r < R; r += (long)gridDim.y * blockDim.y) {
    Vec<V> t, d, o, gx, gr;
    t.load(x + r * ld + c0);
    d.load(dy + r * C + c0);
    if (relu) o.load(y + r * C + c0);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float g = (relu && !(o.v[e] > 0.f)) ? 0.f : d.v[e];
      const float h = (t.v[e] - mu.v[e]) * rs.v[e];
      gx.v[e] = ga.v[e] * (g - A.v[e] - h * B.v[e]);
      gr.v[e] = g;
    }
    gx.store(dx + r * C + c0);
    if (RES) gr.store(dres + r * C + c0);
  }
}

int bn_check(long R, int C, long ld, const char* what) {
  JTSM_REQUIRE(R >= 0 && C > 0 && ld >= C, "%s: need rows >= 0, C > 0 and a leading dimension >= C (R=%ld C=%d ld=%ld)",
               what, R, C, ld);
  JTSM_REQUIRE(R < (1L << 40) && C <= (1 << 20), "%s: map too large (R=%ld C=%d)", what, R, C);
  return JTSM_OK;
}

inline dim3 bn_apply_grid(const BnGeom& g, long R) {
  long gy = (R + g.ty - 1) / g.ty;
  const long cap = 4096 / g.gx > 1 ? 4096 / g.gx : 1;
  if (gy > cap) gy = cap;
  if (gy < 1) gy = 1;
  return dim3(g.gx, (unsigned)gy);
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" {

size_t jtsm_batch_norm_workspace_bytes(long R, int C) {
  if (R <= 0 || C <= 0) return 16;
  const BnGeom a = bn_geom(R, C, false), b = bn_geom(R, C, C % 4 == 0);
  const int slabs = a.slabs > b.slabs ? a.slabs : b.slabs;
  return a16((size_t)slabs * 2 * C * sizeof(double)) + 16;
}

int jtsm_batch_norm_stats_f32(const float* x, long ld, long R, int C, float* mean, float* m2, float eps, float momentum,
                              float* invstd, float* running_mean, float* running_var, void* workspace, void* stream) {
  int rc = bn_check(R, C, ld, "batch_norm_stats");
  if (rc) return rc;
  JTSM_REQUIRE(R > 0, "batch_norm_stats: no rows");
  JTSM_REQUIRE(x && mean && m2 && workspace, "batch_norm_stats: null pointer");
  JTSM_REQUIRE(!invstd || R > 1 || !running_var, "batch_norm_stats: the unbiased variance needs more than one value per channel");
  hipStream_t st = as_stream(stream);
  const bool vec = bn_vec_ok(C, ld, x);
  const BnGeom g = bn_geom(R, C, vec);
  double* part = reinterpret_cast<double*>(workspace);
  if (vec)
    hipLaunchKernelGGL(bn_stats_kernel<4>, dim3(g.gx, g.slabs), dim3(g.tx, g.ty), 0, st, x, ld, R, C, g.rps, part);
  else
    hipLaunchKernelGGL(bn_stats_kernel<1>, dim3(g.gx, g.slabs), dim3(g.tx, g.ty), 0, st, x, ld, R, C, g.rps, part);
  hipLaunchKernelGGL(bn_fold_kernel, dim3((C + FOLD_TC - 1) / FOLD_TC), dim3(256), 0, st, part, R, C, g.rps, g.slabs, mean, m2, eps,
                     momentum, invstd, running_mean, running_var);
  JTSM_CHECK_LAUNCH("batch_norm_stats");
  return JTSM_OK;
}

int jtsm_batch_norm_finalize_f32(const float* mean, const float* m2, double count, int C, float eps, float momentum,
                                 float* invstd, float* running_mean, float* running_var, void* stream) {
  JTSM_REQUIRE(C > 0 && count >= 1.0, "batch_norm_finalize: need C > 0 and a count >= 1");
  JTSM_REQUIRE(mean && m2 && invstd, "batch_norm_finalize: null pointer");
  JTSM_REQUIRE(count > 1.0 || !running_var, "batch_norm_finalize: the unbiased variance needs more than one value per channel");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, as_stream(stream), mean, m2, count, C, eps,
                     momentum, invstd, running_mean, running_var);
  JTSM_CHECK_LAUNCH("batch_norm_finalize");
  return JTSM_OK;
}

int jtsm_batch_norm_apply_f32(const float* x, long ld, const float* residual, const float* mean, const float* invstd,
                              const float* gamma, const float* beta, float* y, long R, int C, int relu, void* stream) {
  int rc = bn_check(R, C, ld, "batch_norm_apply");
  if (rc) return rc;
  if (R == 0) return JTSM_OK;
  JTSM_REQUIRE(x && mean && invstd && gamma && beta && y, "batch_norm_apply: null pointer");
  hipStream_t st = as_stream(stream);
  const bool vec = bn_vec_ok(C, ld, x, residual, y) && bn_vec_ok(C, ld, mean, invstd, gamma, beta);
  const BnGeom g = bn_geom(R, C, vec);
  const dim3 grid = bn_apply_grid(g, R), block(g.tx, g.ty);
#define JTSM_BN_APPLY(V, RES) \
  hipLaunchKernelGGL((bn_apply_kernel<V, RES>), grid, block, 0, st, x, ld, residual, mean, invstd, gamma, beta, y, R, C, relu)
  if (vec) { if (residual) JTSM_BN_APPLY(4, true); else JTSM_BN_APPLY(4, false); }
  else     { if (residual) JTSM_BN_APPLY(1, true); else JTSM_BN_APPLY(1, false); }
#undef JTSM_BN_APPLY
  JTSM_CHECK_LAUNCH("batch_norm_apply");
  return JTSM_OK;
}

int jtsm_batch_norm_backward_reduce_f32(const float* x, long ld, const float* dy, const float* y, const float* mean,
                                        const float* invstd, float* sum_dy, float* sum_dy_xhat, void* workspace, long R,
                                        int C, int relu, void* stream) {
  int rc = bn_check(R, C, ld, "batch_norm_backward_reduce");
  if (rc) return rc;
  JTSM_REQUIRE(R > 0, "batch_norm_backward_reduce: no rows");
  JTSM_REQUIRE(x && dy && mean && invstd && sum_dy && sum_dy_xhat && workspace && (y || !relu),
               "batch_norm_backward_reduce: null pointer (y is needed where the forward applied the ReLU)");
  hipStream_t st = as_stream(stream);
  const bool vec = bn_vec_ok(C, ld, x, dy, y) && bn_vec_ok(C, ld, mean, invstd);
  const BnGeom g = bn_geom(R, C, vec);
  double* part = reinterpret_cast<double*>(workspace);
  if (vec)
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<4>, dim3(g.gx, g.slabs), dim3(g.tx, g.ty), 0, st, x, ld, dy, y, mean, invstd,
                       R, C, g.rps, relu, part);
  else
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<1>, dim3(g.gx, g.slabs), dim3(g.tx, g.ty), 0, st, x, ld, dy, y, mean, invstd,
                       R, C, g.rps, relu, part);
  hipLaunchKernelGGL(bn_bwd_fold_kernel, dim3((C + FOLD_TC - 1) / FOLD_TC), dim3(256), 0, st, part, C, g.slabs, sum_dy, sum_dy_xhat);
  JTSM_CHECK_LAUNCH("batch_norm_backward_reduce");
  return JTSM_OK;
}

int jtsm_batch_norm_backward_apply_f32(const float* x, long ld, const float* dy, const float* y, const float* mean,
                                       const float* invstd, const float* gamma, const float* sum_dy,
                                       const float* sum_dy_xhat, double count, float* dx, float* dresidual, long R, int C,
                                       int relu, void* stream) {
  int rc = bn_check(R, C, ld, "batch_norm_backward_apply");
  if (rc) return rc;
  if (R == 0) return JTSM_OK;
  JTSM_REQUIRE(x && dy && mean && invstd && gamma && sum_dy && sum_dy_xhat && dx && (y || !relu) && count >= 1.0,
               "batch_norm_backward_apply: null pointer or no count");
  hipStream_t st = as_stream(stream);
  const bool vec = bn_vec_ok(C, ld, x, dy, y, dx) && bn_vec_ok(C, ld, mean, invstd, gamma, sum_dy) &&
                   bn_vec_ok(C, ld, sum_dy_xhat, dresidual);
  const BnGeom g = bn_geom(R, C, vec);
  const dim3 grid = bn_apply_grid(g, R), block(g.tx, g.ty);
  const float inv_n = (float)(1.0 / count);
#define JTSM_BN_BWD(V, RES)                                                                                            \
  hipLaunchKernelGGL((bn_bwd_apply_kernel<V, RES>), grid, block, 0, st, x, ld, dy, y, mean, invstd, gamma, sum_dy,     \
                     sum_dy_xhat, inv_n, dx, dresidual, R, C, relu)
  if (vec) { if (dresidual) JTSM_BN_BWD(4, true); else JTSM_BN_BWD(4, false); }
  else     { if (dresidual) JTSM_BN_BWD(1, true); else JTSM_BN_BWD(1, false); }
#undef JTSM_BN_BWD
  JTSM_CHECK_LAUNCH("batch_norm_backward_apply");
  return JTSM_OK;
}

}  // extern "C"
