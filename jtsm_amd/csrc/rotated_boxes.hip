// Rotated boxes (cx, cy, w, h, angle in degrees, counter-clockwise): pairwise IoU and greedy per-class NMS.
// Replaces detectron2/layers/csrc/box_iou_rotated (box_iou_rotated_cuda.cu) and .../nms_rotated (nms_rotated_cuda.cu).
//
// Arithmetic contract: the DEVICE branch of box_iou_rotated_utils.h with every operation rounded on its own (this file
// is built with -ffp-contract=off), its types included: the angle in radians, its cosine and sine are double and cast
// to float; the centre shift is (float + float) / 2.0 in double, subtracted in double, stored to float; EPS = 1e-5 is
// a double and every comparison against it, against 1e-14, 1e-6 and 1e-8 is made in double; the rest is fp32.
// The hull's sort is the header's exchange sort by cross product (ties within 1e-6 by the squared distance taken
// BEFORE the sort), its scan compares the two rounded products.  tests/rotated_ref.py restates the same in NumPy.
//
// Where the per-pair arrays live: up to 24 candidate points, their squared distances and the sort's
// dynamic indexing would put 288 bytes per lane into scratch.  They live in LDS instead, point i of lane l at
// [i * 64 + l] (consecutive lanes, consecutive words: no bank conflict), and the hull works in place — the shifted
// points overwrite the candidates, which nothing reads afterwards: 24 * (8 + 4) B * 64 lanes = 18 KB per wavefront.
// There is no early exit for far-apart pairs: with nearly parallel collinear edges the header's t1 / t2 are rounding
// noise over a tiny determinant, so "centres far apart" does not prove that the reference finds no points.
#include "common.h"
#include "nms_stages.h"

#include <cstdint>

namespace jtsm {
namespace {

struct RBox { float x, y, w, h, a; };
struct Pt { float x, y; };

__device__ __forceinline__ Pt operator-(Pt a, Pt b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ float dot2(Pt a, Pt b) { return a.x * b.x + a.y * b.y; }
__device__ __forceinline__ float cross2(Pt a, Pt b) { return a.x * b.y - b.x * a.y; }

__device__ __forceinline__ void rotated_vertices(const RBox& b, Pt (&p)[4]) {
  const double theta = (double)b.a * 0.01745329251;
  const float c2 = (float)cos(theta) * 0.5f, s2 = (float)sin(theta) * 0.5f;
  p[0].x = b.x + s2 * b.h + c2 * b.w;
  p[0].y = b.y + c2 * b.h - s2 * b.w;
  p[1].x = b.x - s2 * b.h + c2 * b.w;
  p[1].y = b.y - c2 * b.h - s2 * b.w;
  p[2].x = 2.f * b.x - p[0].x;
  p[2].y = 2.f * b.y - p[0].y;
  p[3].x = 2.f * b.x - p[1].x;
  p[3].y = 2.f * b.y - p[1].y;
}

// vertices of `a` that lie inside rectangle `b` (edges vb), appended to the candidates
__device__ __forceinline__ int vertices_inside(const Pt (&a)[4], const Pt (&b)[4], const Pt (&vb)[4], Pt* P, int num) {
  const double EPS = 1e-5;
  const Pt AB = vb[0], DA = vb[3];
  const float ABdotAB = dot2(AB, AB), ADdotAD = dot2(DA, DA);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const Pt AP = a[i] - b[0];
    const float APdotAB = dot2(AP, AB), APdotAD = -dot2(AP, DA);
    if ((double)APdotAB > -EPS && (double)APdotAD > -EPS && (double)APdotAB < (double)ABdotAB + EPS &&
        (double)APdotAD < (double)ADdotAD + EPS) {
      P[num * 64] = a[i];
      ++num;
    }
  }
  return num;
}

// single_box_iou_rotated.  P (24 points) and D (24 distances) are this lane's LDS slices, element i at [i * 64].
__device__ float rotated_iou(const float* __restrict__ r1, const float* __restrict__ r2, Pt* P, float* D) {
#pragma clang fp contract(off)
  const double EPS = 1e-5;
  RBox b1, b2;
  const double shift_x = (double)(r1[0] + r2[0]) / 2.0, shift_y = (double)(r1[1] + r2[1]) / 2.0;
  b1.x = (float)((double)r1[0] - shift_x);
  b1.y = (float)((double)r1[1] - shift_y);
  b1.w = r1[2]; b1.h = r1[3]; b1.a = r1[4];
  b2.x = (float)((double)r2[0] - shift_x);
  b2.y = (float)((double)r2[1] - shift_y);
  b2.w = r2[2]; b2.h = r2[3]; b2.a = r2[4];
  const float area1 = b1.w * b1.h, area2 = b2.w * b2.h;
  if ((double)area1 < 1e-14 || (double)area2 < 1e-14) return 0.f;

  Pt p1[4], p2[4], v1[4], v2[4];
  rotated_vertices(b1, p1);
  rotated_vertices(b2, p2);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v1[i] = p1[(i + 1) & 3] - p1[i];
    v2[i] = p2[(i + 1) & 3] - p2[i];
  }

  // candidates: edge crossings, then vertices of box 1 inside box 2, then vertices of box 2 inside box 1
  int num = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float det = cross2(v2[j], v1[i]);
      if (fabs((double)det) <= 1e-14) continue;   // parallel edges
      const Pt v12 = p2[j] - p1[i];
      const float t1 = cross2(v2[j], v12) / det, t2 = cross2(v1[i], v12) / det;
      if ((double)t1 > -EPS && (double)t1 < 1.0 + EPS && (double)t2 > -EPS && (double)t2 < 1.0 + EPS) {
        P[num * 64] = {p1[i].x + v1[i].x * t1, p1[i].y + v1[i].y * t1};
        ++num;
      }
    }
  }
  num = vertices_inside(p1, p2, v2, P, num);
  num = vertices_inside(p2, p1, v1, P, num);
  if (num <= 2) return 0.f;

  // convex hull (Graham), shifted to its lowest-then-leftmost point, in place
  int t = 0;
  Pt start = P[0];
  for (int i = 1; i < num; ++i) {
    const Pt c = P[i * 64];
    if (c.y < start.y || (c.y == start.y && c.x < start.x)) { t = i; start = c; }
  }
  for (int i = 0; i < num; ++i) {
    const Pt q = P[i * 64] - start;
    P[i * 64] = q;
  }
  {
    const Pt tmp = P[0];
    P[0] = P[t * 64];
    P[t * 64] = tmp;
  }
  for (int i = 0; i < num; ++i) {
    const Pt q = P[i * 64];
    D[i * 64] = dot2(q, q);
  }
  for (int i = 1; i < num - 1; ++i) {
    Pt qi = P[i * 64];
    float di = D[i * 64];
    for (int j = i + 1; j < num; ++j) {
      const Pt qj = P[j * 64];
      const float dj = D[j * 64];
      const float cp = cross2(qi, qj);
      if ((double)cp < -1e-6 || (fabs((double)cp) < 1e-6 && di > dj)) {
        P[j * 64] = qi; D[j * 64] = di;
        qi = qj; di = dj;
      }
    }
    P[i * 64] = qi; D[i * 64] = di;
  }
  int k = 1;
  while (k < num && !((double)D[k * 64] > 1e-8)) ++k;
  if (k == num) return 0.f;   // the hull is one point
  P[64] = P[k * 64];
  int m = 2;
  for (int i = k + 1; i < num; ++i) {
    const Pt qi = P[i * 64];
    while (m > 1) {
      const Pt base = P[(m - 2) * 64];
      const Pt q1 = qi - base, q2 = P[(m - 1) * 64] - base;
      if (q1.x * q2.y >= q2.x * q1.y) --m; else break;
    }
    P[m * 64] = qi;
    ++m;
  }
  if (m <= 2) return 0.f;
  float area = 0.f;
  const Pt q0 = P[0];
  for (int i = 1; i < m - 1; ++i) area += fabsf(cross2(P[i * 64] - q0, P[(i + 1) * 64] - q0));
  const float inter = (float)((double)area / 2.0);
  return inter / (area1 + area2 - inter);
}

constexpr int kPts = 24;

// ious[i, j] for one row i and 64 consecutive columns per one-wavefront workgroup; the (row, column tile) pair is the
// flat workgroup index, so N * M is not bounded by a grid dimension.
__global__ __launch_bounds__(64) void box_iou_rotated_kernel(const float* __restrict__ boxes1,
                                                             const float* __restrict__ boxes2, int N, int M, int tiles,
                                                             float* __restrict__ ious) {
  __shared__ Pt P[kPts * 64];
  __shared__ float D[kPts * 64];
  const int i = blockIdx.x / tiles, j = (blockIdx.x % tiles) * 64 + threadIdx.x;
  if (i >= N || j >= M) return;
  float a[5], b[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) { a[k] = boxes1[(size_t)i * 5 + k]; b[k] = boxes2[(size_t)j * 5 + k]; }
  ious[(size_t)i * M + j] = rotated_iou(a, b, P + threadIdx.x, D + threadIdx.x);
}

// elements of a batched_nms_rotated call (idxs == nullptr: one class)
__global__ __launch_bounds__(256) void rnms_elements_kernel(const float* __restrict__ boxes,
                                                            const float* __restrict__ scores,
                                                            const int64_t* __restrict__ idxs, int n, int K,
                                                            float* __restrict__ ebox, float* __restrict__ escore,
                                                            int* __restrict__ eclass) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int64_t c = idxs ? idxs[e] : 0;
  for (int k = 0; k < 5; ++k) ebox[(size_t)e * 5 + k] = boxes[(size_t)e * 5 + k];
  escore[e] = scores[e];
  eclass[e] = (c >= 0 && c < K) ? (int)c : K;
}

// The bits stage: one 64x64 tile per wavefront, the 64 column boxes staged in LDS, one lane per row, one word per
// lane.  Bit j of row p's word y: sorted element (rb + y) * 64 + j has p's class, comes after p and overlaps it by
// more than thr (`>`, as nms_rotated_cuda.cu; the reference's CPU kernel has `>=`).
__global__ __launch_bounds__(64) void rnms_bits_kernel(const float* __restrict__ ebox, const u64* __restrict__ keys,
                                                       const int* __restrict__ sidx, int N, int K, int W, float thr,
                                                       u64* __restrict__ mask) {
  __shared__ Pt P[kPts * 64];
  __shared__ float D[kPts * 64];
  __shared__ float cbox[64][5];
  __shared__ int ccls[64];
  const int rb = blockIdx.x, y = blockIdx.y, t = threadIdx.x;
  const int p = rb * 64 + t, cb = rb + y;
  u64 bits = 0;
  const int col0 = cb * 64;
  // uniform early-outs: no column, rows all dropped, or the last row's class precedes the first column's class
  const int row_first_cls = rb * 64 < N ? (int)(keys[rb * 64] >> 32) : K;
  bool live = col0 < N && row_first_cls < K;
  if (live) {
    const int last = min(rb * 64 + 63, N - 1);
    live = (int)(keys[col0] >> 32) <= (int)(keys[last] >> 32);
  }
  if (live) {
    const int q = col0 + t;
    int qc = K;
    if (q < N) {
      qc = (int)(keys[q] >> 32);
      const float* src = ebox + (size_t)sidx[q] * 5;
      for (int k = 0; k < 5; ++k) cbox[t][k] = src[k];
    }
    ccls[t] = qc;
    __syncthreads();
    if (p < N) {
      const int pc = (int)(keys[p] >> 32);
      if (pc < K) {
        float a[5];
        const float* src = ebox + (size_t)sidx[p] * 5;
        for (int k = 0; k < 5; ++k) a[k] = src[k];
        const int j0 = y == 0 ? t + 1 : 0;   // strictly upper triangle
        for (int j = j0; j < 64; ++j) {
          if (ccls[j] != pc) continue;
          float b[5];
          for (int k = 0; k < 5; ++k) b[k] = cbox[j][k];
          if (rotated_iou(a, b, P + t, D + t) > thr) bits |= 1ull << j;
        }
      }
    }
  }
  mask[(size_t)p * W + y] = bits;
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" {

int jtsm_box_iou_rotated_f32(const float* boxes1, const float* boxes2, int N, int M, float* ious, void* stream) {
  JTSM_REQUIRE(N >= 0 && M >= 0, "box_iou_rotated: bad sizes N=%d M=%d", N, M);
  if (N == 0 || M == 0) return JTSM_OK;
  JTSM_REQUIRE(boxes1 && boxes2 && ious, "box_iou_rotated: null pointer");
  const int tiles = ceil_div(M, 64);
  JTSM_REQUIRE((long)N * tiles <= 2147483647L, "box_iou_rotated: N * ceil(M / 64) must fit a grid dimension");
  hipLaunchKernelGGL(box_iou_rotated_kernel, dim3((unsigned)((long)N * tiles)), dim3(64), 0, as_stream(stream), boxes1,
                     boxes2, N, M, tiles, ious);
  JTSM_CHECK_LAUNCH("box_iou_rotated");
  return JTSM_OK;
}

size_t jtsm_batched_nms_rotated_workspace_bytes(int n, int num_classes, int max_per_class) {
  if (n <= 0 || num_classes <= 0) return 256;
  Arena a{nullptr};
  carve(a, n, num_classes, max_per_class, 0, 20);
  return a.off;
}

int jtsm_batched_nms_rotated_f32(const float* boxes, const float* scores, const int64_t* idxs, int n, int num_classes,
                                 int max_per_class, float iou_threshold, int64_t* keep, int32_t* num_keep,
                                 int32_t* overflow, void* workspace, size_t workspace_bytes, void* stream) {
  JTSM_REQUIRE(n >= 0 && num_classes >= 1 && max_per_class >= 0, "batched_nms_rotated: bad sizes");
  JTSM_REQUIRE(idxs || num_classes == 1, "batched_nms_rotated: idxs == NULL means one class");
  JTSM_REQUIRE(num_keep, "batched_nms_rotated: num_keep is null");
  hipStream_t st = as_stream(stream);
  if (n == 0) {
    JTSM_CHECK_HIP(hipMemsetAsync(num_keep, 0, sizeof(int32_t), st));
    if (overflow) JTSM_CHECK_HIP(hipMemsetAsync(overflow, 0, sizeof(int32_t), st));
    return JTSM_OK;
  }
  JTSM_REQUIRE(boxes && scores && keep, "batched_nms_rotated: null pointer");
  Arena arena{static_cast<char*>(workspace)};
  const NmsWs w = carve(arena, n, num_classes, max_per_class, 0, 20);
  JTSM_REQUIRE(workspace && workspace_bytes >= arena.off && ((size_t)workspace & 255) == 0,
               "batched_nms_rotated: workspace of %zu bytes (256-byte aligned) needed", arena.off);
  JTSM_REQUIRE((size_t)2 * w.W * 8 <= 64 * 1024, "batched_nms_rotated: max_per_class %d too large", max_per_class);
  float* ebox = static_cast<float*>(w.ebox);
  hipLaunchKernelGGL(nms_header_init, dim3(1), dim3(1), 0, st, w.header);
  hipLaunchKernelGGL(rnms_elements_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, boxes, scores, idxs, n, num_classes,
                     ebox, w.escore, w.eclass);
  JTSM_CHECK_LAUNCH("nms rotated elements");
  const int rc = nms_stages(w, st, [&](const u64* keys, const int* sidx, NmsHeader*, u64* mask) {
    hipLaunchKernelGGL(rnms_bits_kernel, dim3(w.nblk, w.W), dim3(64), 0, st, ebox, keys, sidx, n, num_classes, w.W,
                       iou_threshold, mask);
    JTSM_CHECK_LAUNCH("nms rotated bits");
    return (int)JTSM_OK;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(nms_emit_keep_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, w.order, n, w.header, keep,
                     num_keep, overflow);
  JTSM_CHECK_LAUNCH("nms rotated emit");
  return JTSM_OK;
}

}  // extern "C"
