// ROILoopPool for gfx950 — ContextLocNet's three-region ROI max-pool.
//
// Replaces ROILoopPool_forward/backward (projects/WSL/wsl/layers/csrc/ROILoopPool/ROILoopPool.h:27-40), whose only
// real implementation is CUDA: RoILoopPoolForward / RoILoopPoolBackward and their host wrappers
// (ROILoopPool_cuda.cu:10-205, 207-249, 252-388).  (ROILoopPool_cpu.cpp is a plain ROIPool with other empty-bin
// rules and is not the contract.)
//
// Contract.  rois (R,5) = (b, x1, y1, x2, y2); output / argmax (3R, C, PH, PW): rows [0,R) the BOX block, [R,2R)
// the FRAME block, [2R,3R) the CONTEXT block, each in roi order.  Per roi, in float, every step rounded on its own
// (FMA contraction off — the chosen reading of `w*ratio - w`):
//   ratio = 1.8f (the host wrapper's double literal passed to a float, :309)
//   w = x2-x1, h = y2-y1; inner = w/ratio, h/ratio; outer = w*ratio, h*ratio
//   inner box = (x1 + (w-w/ratio)/2, y1 + ..., x2 - (w-w/ratio)/2, y2 - ...)
//   outer box = (x1 - (w*ratio-w)/2, y1 - ..., x2 + (w*ratio-w)/2, y2 + ...)
//   both clamped to [0, (float)(1.0*W/scale)] x [0, (float)(1.0*H/scale)] (bound in double, then cast)
//   integer rectangles: roundf(coord * scale) (half away from zero)
//   bins: width max(end-start+1, 1); [floor(p*bin), ceil((p+1)*bin)) + start, clipped to the map
//   box + frame: one scan of the box's bin (h outer, w inner, strict '>'), both maxima start at 0, argmax -1 (the
//     reference's "assume all input is >= 0": an all-zero or all-negative bin gives 0 / -1); a cell counts for the
//     frame unless in_y0 < h < in_y1 && in_x0 < w < in_x1 (inner box's rectangle; its border belongs to the frame)
//   context: scan of the outer box's bin, cells strictly inside the box's own rectangle skipped (same strict test)
//   argmax: flat h*W + w in the (image, channel) plane.
// Backward: grad_in[b, c, argmax] += grad_out[n, c, ph, pw] over all three blocks (image of row n: rois[n % R]).
//
// Forward (NHWC): one wavefront per (roi, bin row); lanes hold channels (4 floats each: 1 KiB per 256-channel row).
// The box and frame maxima come out of one pass over the box's bin rows, the context block out of a second pass over
// the outer box's bin rows.  NCHW: one thread per (roi, channel, bin), the reference's mapping.
// Backward (NHWC): a GATHER — one wavefront per (image, cell) and 256-channel block walks the rois in index order,
// finds the (roi, block, bin) triples whose bin holds the cell from the integer geometry alone (precomputed per roi
// by a small kernel) and adds the gradients whose argmax names the cell.  Every cell is written once, no atomics: two
// calls on the same inputs give the same bits.
#include "pool_bins.h"

namespace jtsm {
namespace {

#pragma clang fp contract(off)

constexpr float kContextRatio = 1.8f;   // ROILoopPool_cuda.cu:309 (a double literal converted to the float parameter)

struct LoopGeom {
  int b;
  int x0, y0, x1, y1;           // the box's integer rectangle
  int ix0, iy0, ix1, iy1;       // the inner box's
  int ox0, oy0, ox1, oy1;       // the outer box's
};

__device__ __forceinline__ LoopGeom loop_geometry(const float* __restrict__ roi, float scale, int H, int W) {
#pragma clang fp contract(off)
  LoopGeom g;
  g.b = (int)roi[0];
  const float x1 = roi[1], y1 = roi[2], x2 = roi[3], y2 = roi[4];
  const float rw = x2 - x1, rh = y2 - y1;
  const float iw = rw / kContextRatio, ih = rh / kContextRatio;
  const float ow = rw * kContextRatio, oh = rh * kContextRatio;
  const float irw = rw - iw, irh = rh - ih;
  const float orw = ow - rw, orh = oh - rh;
  const float bx = (float)(1.0 * W / (double)scale), by = (float)(1.0 * H / (double)scale);
  auto cl = [](float v, float hi) { return fminf(fmaxf(v, 0.f), hi); };
  const float x1i = cl(x1 + irw / 2.f, bx), y1i = cl(y1 + irh / 2.f, by);
  const float x2i = cl(x2 - irw / 2.f, bx), y2i = cl(y2 - irh / 2.f, by);
  const float x1o = cl(x1 - orw / 2.f, bx), y1o = cl(y1 - orh / 2.f, by);
  const float x2o = cl(x2 + orw / 2.f, bx), y2o = cl(y2 + orh / 2.f, by);
  g.x0 = (int)roundf(x1 * scale);  g.y0 = (int)roundf(y1 * scale);
  g.x1 = (int)roundf(x2 * scale);  g.y1 = (int)roundf(y2 * scale);
  g.ix0 = (int)roundf(x1i * scale); g.iy0 = (int)roundf(y1i * scale);
  g.ix1 = (int)roundf(x2i * scale); g.iy1 = (int)roundf(y2i * scale);
  g.ox0 = (int)roundf(x1o * scale); g.oy0 = (int)roundf(y1o * scale);
  g.ox1 = (int)roundf(x2o * scale); g.oy1 = (int)roundf(y2o * scale);
  return g;
}

// One wavefront per (roi, bin row ph); lane owns channels [c, c + VEC) of every 64*VEC-channel block.
template <int VEC>
__global__ __launch_bounds__(256) void loop_pool_fwd_nhwc(const float* __restrict__ in, const float* __restrict__ rois,
                                                          float* __restrict__ out, int* __restrict__ argmax, int B, int C,
                                                          int H, int W, int R, float scale, int PH, int PW) {
#pragma clang fp contract(off)
  using V = typename VecT<VEC>::T;
  const long wave = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (wave >= (long)R * PH) return;
  const int lane = threadIdx.x & 63;
  const int n = (int)(wave / PH), ph = (int)(wave - (long)n * PH);
  const LoopGeom g = loop_geometry(rois + (size_t)n * 5, scale, H, W);
  const bool ok = g.b >= 0 && g.b < B;            // (a roi naming no image pools nothing: 0 / -1)
  const float* __restrict__ img = in + (size_t)(ok ? g.b : 0) * H * W * C;
  const size_t block = (size_t)R * PH * PW * C;   // elements of one of the three blocks
  const float bbh = bin_size(g.y0, g.y1, PH), bbw = bin_size(g.x0, g.x1, PW);
  const float obh = bin_size(g.oy0, g.oy1, PH), obw = bin_size(g.ox0, g.ox1, PW);
  const int bhs = clampi(bin_lo(ph, bbh, g.y0), 0, H), bhe = ok ? clampi(bin_hi(ph, bbh, g.y0), 0, H) : 0;
  const int ohs = clampi(bin_lo(ph, obh, g.oy0), 0, H), ohe = ok ? clampi(bin_hi(ph, obh, g.oy0), 0, H) : 0;
  for (int c = lane * VEC; c < C; c += 64 * VEC) {
    for (int pw = 0; pw < PW; ++pw) {
      const size_t o = (((size_t)n * PH + ph) * PW + pw) * C + c;
      // ---- box + frame: one scan of the box's bin
      {
        const int ws = clampi(bin_lo(pw, bbw, g.x0), 0, W), we = clampi(bin_hi(pw, bbw, g.x0), 0, W);
        V mb, mf;
        int ab[VEC], af[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) { set_comp(mb, k, 0.f); set_comp(mf, k, 0.f); ab[k] = -1; af[k] = -1; }
        for (int h = bhs; h < bhe; ++h) {
          const bool in_h = h > g.iy0 && h < g.iy1;
          const float* __restrict__ row = img + (size_t)h * W * C + c;
#pragma unroll 4
          for (int w = ws; w < we; ++w) {
            const V v = *reinterpret_cast<const V*>(row + (size_t)w * C);
            const bool frame = !(in_h && w > g.ix0 && w < g.ix1);
            const int idx = h * W + w;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {   // (update_max of both maxima, one pass over the lane's channels)
              const float x = comp(v, k);
              if (x > comp(mb, k)) { set_comp(mb, k, x); ab[k] = idx; }
              if (frame && x > comp(mf, k)) { set_comp(mf, k, x); af[k] = idx; }
            }
          }
        }
        *reinterpret_cast<V*>(out + o) = mb;
        *reinterpret_cast<V*>(out + block + o) = mf;
#pragma unroll
        for (int k = 0; k < VEC; ++k) { argmax[o + k] = ab[k]; argmax[block + o + k] = af[k]; }
      }
      // ---- context: the outer box's bin minus the box's strict interior
      {
        const int ws = clampi(bin_lo(pw, obw, g.ox0), 0, W), we = clampi(bin_hi(pw, obw, g.ox0), 0, W);
        V mc;
        int ac[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) { set_comp(mc, k, 0.f); ac[k] = -1; }
        for (int h = ohs; h < ohe; ++h) {
          const bool in_h = h > g.y0 && h < g.y1;
          const float* __restrict__ row = img + (size_t)h * W * C + c;
#pragma unroll 4
          for (int w = ws; w < we; ++w) {
            if (in_h && w > g.x0 && w < g.x1) continue;
            const V v = *reinterpret_cast<const V*>(row + (size_t)w * C);
            update_max<VEC>(v, h * W + w, mc, ac);
          }
        }
        *reinterpret_cast<V*>(out + 2 * block + o) = mc;
#pragma unroll
        for (int k = 0; k < VEC; ++k) argmax[2 * block + o + k] = ac[k];
      }
    }
  }
}

// NCHW: one thread per (roi, channel, bin), as RoILoopPoolForward maps it.
__global__ __launch_bounds__(256) void loop_pool_fwd_nchw(const float* __restrict__ in, const float* __restrict__ rois,
                                                          float* __restrict__ out, int* __restrict__ argmax, int B, int C,
                                                          int H, int W, int R, float scale, int PH, int PW) {
#pragma clang fp contract(off)
  const long total = (long)R * C * PH * PW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int pw = (int)(i % PW), ph = (int)((i / PW) % PH), c = (int)((i / PW / PH) % C), n = (int)(i / PW / PH / C);
    const LoopGeom g = loop_geometry(rois + (size_t)n * 5, scale, H, W);
    const bool ok = g.b >= 0 && g.b < B;
    const float* __restrict__ p = in + ((size_t)(ok ? g.b : 0) * C + c) * H * W;
    {
      const float bh = bin_size(g.y0, g.y1, PH), bw = bin_size(g.x0, g.x1, PW);
      const int hs = clampi(bin_lo(ph, bh, g.y0), 0, H), he = ok ? clampi(bin_hi(ph, bh, g.y0), 0, H) : 0;
      const int ws = clampi(bin_lo(pw, bw, g.x0), 0, W), we = clampi(bin_hi(pw, bw, g.x0), 0, W);
      float mb = 0.f, mf = 0.f;
      int ab = -1, af = -1;
      for (int h = hs; h < he; ++h)
        for (int w = ws; w < we; ++w) {
          const int idx = h * W + w;
          const float x = p[idx];
          update_max(x, idx, mb, ab);
          if (h > g.iy0 && h < g.iy1 && w > g.ix0 && w < g.ix1) continue;
          update_max(x, idx, mf, af);
        }
      out[i] = mb; argmax[i] = ab;
      out[total + i] = mf; argmax[total + i] = af;
    }
    {
      const float bh = bin_size(g.oy0, g.oy1, PH), bw = bin_size(g.ox0, g.ox1, PW);
      const int hs = clampi(bin_lo(ph, bh, g.oy0), 0, H), he = ok ? clampi(bin_hi(ph, bh, g.oy0), 0, H) : 0;
      const int ws = clampi(bin_lo(pw, bw, g.ox0), 0, W), we = clampi(bin_hi(pw, bw, g.ox0), 0, W);
      float mc = 0.f;
      int ac = -1;
      for (int h = hs; h < he; ++h)
        for (int w = ws; w < we; ++w) {
          if (h > g.y0 && h < g.y1 && w > g.x0 && w < g.x1) continue;
          update_max(p[h * W + w], h * W + w, mc, ac);
        }
      out[2 * total + i] = mc; argmax[2 * total + i] = ac;
    }
  }
}

// Per-roi record of the backward gather: image, the box's rectangle (blocks 0, 1) and the outer box's (block 2).
struct LoopReach {
  int b;
  BinRect box, outer;
  int pad[3];
};
static_assert(sizeof(LoopReach) == 64, "LoopReach is one 64-byte record");

__global__ __launch_bounds__(256) void loop_pool_reach_kernel(const float* __restrict__ rois, LoopReach* __restrict__ reach,
                                                              int R, int H, int W, float scale, int PH, int PW) {
#pragma clang fp contract(off)
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= R) return;
  const LoopGeom g = loop_geometry(rois + (size_t)n * 5, scale, H, W);
  reach[n] = {g.b, BinRect(g.x0, g.y0, g.x1, g.y1, PH, PW), BinRect(g.ox0, g.oy0, g.ox1, g.oy1, PH, PW), {0, 0, 0}};
}

// grad_in[b, h, w, c] = sum over (roi n, block k, bin (ph, pw)) whose bin holds (h, w) and whose argmax names it of
// grad[kR + n, ph, pw, c] — roi order, then the box's bins (block 0, then block 1 of each bin), then the outer box's
// (block 2): a fixed order.  One wavefront per (image, cell) and 64*VEC-channel block (grid.y).
template <int VEC>
__global__ __launch_bounds__(256) void loop_pool_bwd_gather(const float* __restrict__ grad, const int* __restrict__ argmax,
                                                            const LoopReach* __restrict__ reach, float* __restrict__ gin,
                                                            int B, int C, int H, int W, int R, int PH, int PW) {
#pragma clang fp contract(off)
  using V = typename VecT<VEC>::T;
  const long cell = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (cell >= (long)B * H * W) return;
  const int lane = threadIdx.x & 63;
  const int w = (int)(cell % W), h = (int)((cell / W) % H), b = (int)(cell / W / H);
  const int c = (blockIdx.y * 64 + lane) * VEC;
  const bool live = c < C;
  const int idx = h * W + w;
  const size_t block = (size_t)R * PH * PW * C;
  float acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
  auto add = [&](size_t row) {   // row = (n', ph, pw) of one block
    if (live) gather_add<VEC>(acc, grad, argmax, row, C, c, idx);
  };
  for (int n = 0; n < R; ++n) {
    const LoopReach q = reach[n];   // (uniform: scalar loads)
    if (q.b != b) continue;
    const bool in_box = q.box.reaches(h, w), in_outer = q.outer.reaches(h, w);
    if (in_box)
      for_bins_holding(q.box, h, w, PH, PW, [&](int ph, int pw) {
        const size_t row = ((size_t)n * PH + ph) * PW + pw;
        add(row);
        add(row + block / C);
      });
    if (in_outer)
      for_bins_holding(q.outer, h, w, PH, PW, [&](int ph, int pw) { add(((size_t)n * PH + ph) * PW + pw + 2 * (block / C)); });
  }
  if (!live) return;
  V v;
#pragma unroll
  for (int k = 0; k < VEC; ++k) set_comp(v, k, acc[k]);
  *reinterpret_cast<V*>(gin + (size_t)cell * C + c) = v;
}

}  // namespace
}  // namespace jtsm

using namespace jtsm;

extern "C" {

int jtsm_roi_loop_pool_forward_f32(const float* input, const float* rois, float* output, int32_t* argmax, int B, int C,
                                   int H, int W, int R, float spatial_scale, int pooled_h, int pooled_w, int layout,
                                   void* stream) {
  return pool_forward<loop_pool_fwd_nhwc<4>, loop_pool_fwd_nhwc<1>, loop_pool_fwd_nchw>(
      "roi_loop_pool", input, rois, output, argmax, B, C, H, W, R, spatial_scale, pooled_h, pooled_w, layout, stream);
}

size_t jtsm_roi_loop_pool_backward_workspace_bytes(int R) { return pool_backward_workspace_bytes<LoopReach>(R); }

int jtsm_roi_loop_pool_backward_f32(const float* grad, const float* rois, const int32_t* argmax, float* grad_input,
                                    void* workspace, int B, int C, int H, int W, int R, float spatial_scale, int pooled_h,
                                    int pooled_w, void* stream) {
  return pool_backward<LoopReach, loop_pool_reach_kernel, loop_pool_bwd_gather<4>, loop_pool_bwd_gather<1>>(
      "roi_loop_pool", grad, rois, argmax, grad_input, workspace, B, C, H, W, R, spatial_scale, pooled_h, pooled_w,
      stream);
}

}  // extern "C"
