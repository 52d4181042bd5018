/*
 * jtsm_hip.h — C ABI of libjtsm_hip.so: the MI355X (gfx950) hot path of JTSM.
 *
 * Every entry point takes plain device pointers, sizes and a hipStream_t passed as
 * void* (NULL = the null stream).  No torch/ATen types cross this boundary.  The
 * library never allocates device memory: outputs and workspaces are caller-owned,
 * exactly sized as documented; inputs are never written.  All launches are
 * asynchronous on `stream`; nothing here synchronises the device (the reference's
 * forward does a cudaDeviceSynchronize, ROIAlign_cuda.cu:364 — deliberately not kept).
 *
 * Return value: 0 on success, a negative JTSM_E* code otherwise;
 * jtsm_last_error() gives the message of the calling thread's last failure.  The
 * reference reports the same conditions as C++ exceptions -> Python RuntimeError
 * (AT_ASSERTM / TORCH_CHECK, e.g. ROIAlign_cuda.cu:318-324); the Python host layer
 * (jtsm_amd/_lib.py) turns a non-zero return into RuntimeError to keep that behaviour.
 *
 * Each group cites the reference interface it replaces (paths relative to the
 * reference tree).  `layout` selects how 4-D feature tensors are stored:
 * JTSM_NCHW is what the reference FFI uses; JTSM_NHWC is the layout the MI355X path
 * keeps activations in (channels across the 64 lanes of a wavefront -> coalesced
 * 1 KiB rows).  Pooled outputs / gradients use the same layout as the feature map:
 * (M,C,PH,PW) for NCHW, (M,PH,PW,C) for NHWC.
 */
#ifndef JTSM_HIP_H_
#define JTSM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JTSM_OK 0
#define JTSM_EINVAL (-1)   /* bad argument (shape, null pointer, unsupported combination) */
#define JTSM_ELAUNCH (-2)  /* HIP runtime reported a launch / API error */
#define JTSM_ENODEV (-3)   /* no gfx950 device / code object not loadable */

#define JTSM_NCHW 0
#define JTSM_NHWC 1

const char* jtsm_last_error(void);
/* "jtsm_hip <version> gfx950" — also proves the shared object is the HIP build. */
const char* jtsm_version(void);
/* Number of visible HIP devices (<0 on error).  Does not create a context. */
int jtsm_device_count(void);

/* Launch timing for measurement harnesses: thin hipEvent wrappers, and a hook that records `event` right after
 * the next contraction kernel launched by the calling thread (before its split-K finishing pass, if any) — the
 * kernel's own duration, as rocprofv3 reports it, without a second process. */
void* jtsm_event_create(void);
int jtsm_event_record(void* event, void* stream);
int jtsm_event_elapsed_ms(void* start, void* stop, float* ms);
void jtsm_event_destroy(void* event);
void jtsm_conv_set_mid_event(void* event);
/* Split-K finishing of the bf16x3 / fp16 contractions: 1 = inside the contraction kernel (the tile's last-arriving K
 * slice folds the slabs in slice order and runs the epilogue: sc1 write-through slab stores, sc1 loads, an agent-scope
 * ticket, no device-scope fence), 0 = the separate splitk_finish pass, -1 = follow JTSM_SPLITK_FUSED (default: 0 — the in-kernel form
 * measured 45 % slower per step on MI355X: its slab traffic goes to HBM instead of staying in L2 / Infinity Cache).
 * Both give bit-identical results (same slice order, same epilogue arithmetic); the switch exists for tests / sweeps. */
void jtsm_conv_set_splitk_fused(int mode);

/* ---------------------------------------------------------------------------
 * ROIAlign — replaces detectron2/layers/csrc/ROIAlign/ROIAlign.h:7-27
 *   ROIAlign_forward(input, rois, spatial_scale, pooled_h, pooled_w, sampling_ratio, aligned)
 *   ROIAlign_backward(grad, rois, spatial_scale, pooled_h, pooled_w, B, C, H, W,
 *                     sampling_ratio, aligned)
 * bound at detectron2/layers/csrc/vision.cpp:96-97, called from
 * detectron2/layers/roi_align.py:22-59.
 * rois: (M,5) [batch_idx, x0, y0, x1, y1], same dtype as input.
 * backward: grad is dense in `layout`; grad_input (B,C,H,W in `layout`) is zero-filled
 * by the call and then accumulated with float atomics.
 * ------------------------------------------------------------------------- */
int jtsm_roi_align_forward_f32(const float* input, const float* rois, float* output, int B,
                               int C, int H, int W, int M, float spatial_scale, int pooled_h,
                               int pooled_w, int sampling_ratio, int aligned, int layout,
                               void* stream);
int jtsm_roi_align_backward_f32(const float* grad, const float* rois, float* grad_input, int B,
                                int C, int H, int W, int M, float spatial_scale, int pooled_h,
                                int pooled_w, int sampling_ratio, int aligned, int layout,
                                void* stream);
int jtsm_roi_align_forward_f64(const double* input, const double* rois, double* output, int B,
                               int C, int H, int W, int M, double spatial_scale, int pooled_h,
                               int pooled_w, int sampling_ratio, int aligned, int layout,
                               void* stream);
int jtsm_roi_align_backward_f64(const double* grad, const double* rois, double* grad_input,
                                int B, int C, int H, int W, int M, double spatial_scale,
                                int pooled_h, int pooled_w, int sampling_ratio, int aligned,
                                int layout, void* stream);

/* ---------------------------------------------------------------------------
 * ROIAlignRotated — replaces detectron2/layers/csrc/ROIAlignRotated/ROIAlignRotated.h:7-27
 * (bound at vision.cpp:99-106, called from detectron2/layers/roi_align_rotated.py:10-47).
 * rois: (M,6) [batch_idx, cx, cy, w, h, angle_degrees]; always "aligned".
 * ------------------------------------------------------------------------- */
int jtsm_roi_align_rotated_forward_f32(const float* input, const float* rois, float* output,
                                       int B, int C, int H, int W, int M, float spatial_scale,
                                       int pooled_h, int pooled_w, int sampling_ratio,
                                       int layout, void* stream);
int jtsm_roi_align_rotated_backward_f32(const float* grad, const float* rois, float* grad_input,
                                        int B, int C, int H, int W, int M, float spatial_scale,
                                        int pooled_h, int pooled_w, int sampling_ratio,
                                        int layout, void* stream);
int jtsm_roi_align_rotated_forward_f64(const double* input, const double* rois, double* output,
                                       int B, int C, int H, int W, int M, double spatial_scale,
                                       int pooled_h, int pooled_w, int sampling_ratio,
                                       int layout, void* stream);
int jtsm_roi_align_rotated_backward_f64(const double* grad, const double* rois,
                                        double* grad_input, int B, int C, int H, int W, int M,
                                        double spatial_scale, int pooled_h, int pooled_w,
                                        int sampling_ratio, int layout, void* stream);

/* The "bit-exact ROI bin indices" contract made observable: for each of the M rois write
 * grid[2m..] = {gh, gw} and, for the first `cap` samples in (ph, pw, iy, ix) order,
 * pos[(m*cap+s)*4..] (flat y*W+x of the 4 taps, -1 when the sample is out of range) and
 * w[(m*cap+s)*4..].  Uses the very device functions the pooling kernels use.
 * rotated=0: rois (M,5) with `aligned`; rotated=1: rois (M,6). */
int jtsm_roi_sample_table_f32(const float* rois, int rotated, int M, int H, int W,
                              float spatial_scale, int pooled_h, int pooled_w,
                              int sampling_ratio, int aligned, int* grid, int* pos, float* w,
                              int cap, void* stream);

/* ---------------------------------------------------------------------------
 * MOIPool — replaces projects/WSL/wsl/layers/csrc/MOIPool/MOIPool.h:7-47
 *   MOIPool_forward(input, rois, spatial_scale, pooled_h, pooled_w, oh_labels, superpixels)
 *       -> (output, argmax)
 *   MOIPool_backward(grad, rois, argmax, spatial_scale, pooled_h, pooled_w, B, C, H, W)
 * bound at projects/WSL/wsl/layers/csrc/vision.cpp:23-24, called from
 * projects/WSL/wsl/layers/moi_pool.py:10-33.
 * rois (M,5); oh_labels (M,L) int32; superpixels (B,Hs,Ws) int32 with ids in [0,L)
 * (ids outside that range never match — the reference reads out of bounds there).
 * argmax holds the flat h*W+w of the winning cell (-1 = empty bin), stored in `layout`
 * like output.  The reference's (M,H,W) int32 `mois` temporary (MOIPool_cuda.cu:394) is
 * replaced by two bit sets kept in `workspace`: one per feature cell (which superpixels
 * lie under it) and one per roi (which superpixels are labelled 1).
 * workspace: jtsm_moi_pool_workspace_bytes(...) bytes, 16-byte aligned, contents
 * undefined on entry and exit.
 * ------------------------------------------------------------------------- */
size_t jtsm_moi_pool_workspace_bytes(int B, int H, int W, int M, int L);
int jtsm_moi_pool_forward_f32(const float* input, const float* rois, const int32_t* oh_labels,
                              const int32_t* superpixels, float* output, int32_t* argmax,
                              void* workspace, int B, int C, int H, int W, int M, int L, int Hs,
                              int Ws, float spatial_scale, int pooled_h, int pooled_w,
                              int layout, void* stream);
int jtsm_moi_pool_backward_f32(const float* grad, const float* rois, const int32_t* argmax,
                               float* grad_input, int B, int C, int H, int W, int M,
                               int pooled_h, int pooled_w, int layout, void* stream);
/* ---------------------------------------------------------------------------
 * ROILoopPool — replaces projects/WSL/wsl/layers/csrc/ROILoopPool/ROILoopPool.h:27-40
 *   ROILoopPool_forward(input, rois, spatial_scale, pooled_h, pooled_w) -> (output, argmax)
 *   ROILoopPool_backward(grad, rois, argmax, spatial_scale, pooled_h, pooled_w, B, C, H, W)
 * called from projects/WSL/wsl/layers/roi_loop_pool.py:9-33 (contract: ROILoopPool_cuda.cu:10-388,
 * spelled out in jtsm_amd/csrc/roi_loop_pool.hip).
 * rois (R,5); output / argmax (3R,C,PH,PW) in `layout`: rows [0,R) box, [R,2R) frame (box minus
 * the shrunken inner box), [2R,3R) context (enlarged outer box minus the box), context ratio 1.8.
 * argmax holds the flat h*W+w of the winning cell (-1 = nothing above 0 in the bin).
 * The backward is NHWC only (grad, argmax, grad_input channels-last) and writes every element of
 * grad_input (no zero fill needed); it is a gather in a fixed order, so repeated calls give the
 * same bits.  workspace: jtsm_roi_loop_pool_backward_workspace_bytes(R) bytes, 16-byte aligned.
 * ------------------------------------------------------------------------- */
int jtsm_roi_loop_pool_forward_f32(const float* input, const float* rois, float* output, int32_t* argmax,
                                   int B, int C, int H, int W, int R, float spatial_scale, int pooled_h,
                                   int pooled_w, int layout, void* stream);
size_t jtsm_roi_loop_pool_backward_workspace_bytes(int R);
int jtsm_roi_loop_pool_backward_f32(const float* grad, const float* rois, const int32_t* argmax,
                                    float* grad_input, void* workspace, int B, int C, int H, int W, int R,
                                    float spatial_scale, int pooled_h, int pooled_w, void* stream);
/* ---------------------------------------------------------------------------
 * ROIPool — replaces torchvision.ops.RoIPool(output_size, spatial_scale)(input, rois) as
 * projects/WSL/wsl/modeling/poolers.py:6,183-186 builds and calls it (PCL's POOLER_TYPE "ROIPool";
 * contract spelled out in jtsm_amd/csrc/roi_pool.hip).
 * rois (R,5); output / argmax (R,C,PH,PW) in `layout`.  Integer rectangle roundf(coord * scale);
 * bins [floor(p*bin), ceil((p+1)*bin)) + start with bin = max(end-start+1, 1) / P, clipped to the
 * map; an empty bin gives 0 / -1, otherwise the first cell (h outer, w inner) holding the maximum.
 * argmax holds the flat h*W+w of the winning cell.
 * The backward is NHWC only (grad, argmax, grad_input channels-last) and writes every element of
 * grad_input; it is a gather in a fixed order, so repeated calls give the same bits.
 * workspace: jtsm_roi_pool_backward_workspace_bytes(R) bytes, 16-byte aligned.
 * ------------------------------------------------------------------------- */
int jtsm_roi_pool_forward_f32(const float* input, const float* rois, float* output, int32_t* argmax,
                              int B, int C, int H, int W, int R, float spatial_scale, int pooled_h,
                              int pooled_w, int layout, void* stream);
size_t jtsm_roi_pool_backward_workspace_bytes(int R);
int jtsm_roi_pool_backward_f32(const float* grad, const float* rois, const int32_t* argmax,
                               float* grad_input, void* workspace, int B, int C, int H, int W, int R,
                               float spatial_scale, int pooled_h, int pooled_w, void* stream);
/* ---------------------------------------------------------------------------
 * fp16 tensors at the pooling boundary.  The reference dispatches MOIPool on half too
 * (AT_DISPATCH_FLOATING_TYPES_AND_HALF, projects/WSL/wsl/layers/csrc/MOIPool/MOIPool_cuda.cu:400,415,484) and its
 * Python layers hand half tensors to the align operators (detectron2/layers/roi_align_rotated.py:79-85: up-cast,
 * compute, cast back).  input / rois / output / grad are IEEE binary16 bit patterns; every call needs a caller
 * workspace (16-byte aligned) in which the values are widened to fp32, pooled by the fp32 kernels above and rounded
 * to fp16 once.  MOIPool is exact (a maximum of fp16 values; roi corners = round(Half(x) * Half(scale)), the product
 * rounded to half as c10::Half arithmetic does); the align operators accumulate in fp32 and round once.
 *   jtsm_pool_f16_workspace_bytes(in, rois, out, extra): elements of the tensor read, of the rois, of the tensor
 *   written (+ extra bytes) — what the align calls need (extra = 0) and the MOIPool backward needs. */
size_t jtsm_pool_f16_workspace_bytes(long in_elems, long roi_elems, long out_elems, size_t extra);
size_t jtsm_moi_pool_f16_workspace_bytes(int B, int C, int H, int W, int M, int L, int pooled_h, int pooled_w);
int jtsm_roi_align_forward_f16(const uint16_t* input, const uint16_t* rois, uint16_t* output, int B, int C, int H, int W,
                               int M, float spatial_scale, int pooled_h, int pooled_w, int sampling_ratio, int aligned,
                               int layout, void* workspace, size_t workspace_bytes, void* stream);
int jtsm_roi_align_backward_f16(const uint16_t* grad, const uint16_t* rois, uint16_t* grad_input, int B, int C, int H,
                                int W, int M, float spatial_scale, int pooled_h, int pooled_w, int sampling_ratio,
                                int aligned, int layout, void* workspace, size_t workspace_bytes, void* stream);
int jtsm_roi_align_rotated_forward_f16(const uint16_t* input, const uint16_t* rois, uint16_t* output, int B, int C,
                                       int H, int W, int M, float spatial_scale, int pooled_h, int pooled_w,
                                       int sampling_ratio, int layout, void* workspace, size_t workspace_bytes,
                                       void* stream);
int jtsm_roi_align_rotated_backward_f16(const uint16_t* grad, const uint16_t* rois, uint16_t* grad_input, int B, int C,
                                        int H, int W, int M, float spatial_scale, int pooled_h, int pooled_w,
                                        int sampling_ratio, int layout, void* workspace, size_t workspace_bytes,
                                        void* stream);
int jtsm_moi_pool_forward_f16(const uint16_t* input, const uint16_t* rois, const int32_t* oh_labels,
                              const int32_t* superpixels, uint16_t* output, int32_t* argmax, void* workspace,
                              size_t workspace_bytes, int B, int C, int H, int W, int M, int L, int Hs, int Ws,
                              float spatial_scale, int pooled_h, int pooled_w, int layout, void* stream);
int jtsm_moi_pool_backward_f16(const uint16_t* grad, const uint16_t* rois, const int32_t* argmax, uint16_t* grad_input,
                               void* workspace, size_t workspace_bytes, int B, int C, int H, int W, int M, int pooled_h,
                               int pooled_w, int layout, void* stream);

/* All FPN levels in ONE launch — what detectron2/modeling/poolers.py:193-250 does level by level around
 * wsl/layers/moi_pool.py:10-33.  inputs[l] / grad_inputs[l]: (B,H[l],W[l],C) NHWC maps (host arrays of device
 * pointers, nlevels <= 8); roi_level[n] in [0,nlevels) picks roi n's map; output / argmax as above (NHWC).
 * Backward: with `scales` (the forward's level scales), a workspace
 * (jtsm_moi_pool_backward_levels_workspace_bytes) and C a multiple of 256, every gradient map is produced by a
 * gather — one workgroup per 8x8-cell tile (per 4x4-cell quadrant of a tile with an estimated 1024 pairs or more)
 * sums, in a fixed order, the gradients of the bins whose argmax fell into it (LDS accumulation, no atomics, bitwise
 * reproducible, every cell written once) — unless a census of the roi boxes estimates more than 64000 (roi, bin)
 * pairs on one tile (proposals piled on one spot), in which case, and otherwise (scales or workspace NULL), each
 * grad_inputs[l] is zero-filled and accumulated with float atomics. */
size_t jtsm_moi_pool_levels_workspace_bytes(int B, const int* H, const int* W, int nlevels, int M, int L);
int jtsm_moi_pool_forward_levels_f32(const float* const* inputs, const int* H, const int* W,
                                     const float* scales, int nlevels, const float* rois,
                                     const int32_t* roi_level, const int32_t* oh_labels,
                                     const int32_t* superpixels, float* output, int32_t* argmax,
                                     void* workspace, int B, int C, int M, int L, int Hs, int Ws,
                                     int pooled_h, int pooled_w, void* stream);
size_t jtsm_moi_pool_backward_levels_workspace_bytes(const int* H, const int* W, int nlevels, int B, int M);
int jtsm_moi_pool_backward_levels_f32(const float* grad, const float* rois, const int32_t* roi_level,
                                      const int32_t* argmax, float* const* grad_inputs, const int* H,
                                      const int* W, const float* scales, int nlevels, int B, int C, int M,
                                      int pooled_h, int pooled_w, int accumulate, void* workspace,
                                      size_t workspace_bytes, void* stream);

/* mois (M,H,W) int32 exactly as MoIForward (MOIPool_cuda.cu:138-215) would write it;
 * test/diagnostic entry, same workspace contract as the forward. */
int jtsm_moi_mask_f32(const float* rois, const int32_t* oh_labels, const int32_t* superpixels,
                      int32_t* mois, void* workspace, int B, int H, int W, int M, int L, int Hs,
                      int Ws, float spatial_scale, void* stream);


/* ---------------------------------------------------------------------------
 * Convolution / linear layers on the fp32 matrix cores (v_mfma_f32_32x32x2_f32).
 * The reference has no source for these: it calls ATen/cuDNN through F.conv2d /
 * nn.Linear at detectron2/layers/wrappers.py:76-78 (Conv2d.forward),
 * detectron2/modeling/backbone/resnet.py:195-211,355-359, fpn.py:127-152,
 * projects/WSL/wsl/modeling/roi_heads/box_head.py:90-93, mask_head.py:339-343,
 * detectron2/modeling/meta_arch/semantic_seg.py:170-177.  These entry points replace that
 * call and fuse what the reference runs as separate passes behind it (FrozenBatchNorm2d
 * affine, batch_norm.py:45-66; shortcut add and ReLU, resnet.py:203-210).
 *
 * Layouts: activations NHWC (batch, h, w, c) dense; weights OHWI = [out_c][kh][kw][in_c]
 * dense (a torch (O,I,kh,kw) weight stored channels_last is exactly this).  nn.Linear's
 * [out][in] weight is the 1x1 case with in_h = in_w = 1, batch = rows.
 * in_c must be a multiple of 4 (pad RGB to 4 channels); backward also needs out_c % 4 == 0.
 * All pointers 16-byte aligned.
 * ------------------------------------------------------------------------- */
typedef struct jtsm_conv_shape {
  int batch, in_h, in_w, in_c; /* input  (batch, in_h, in_w, in_c)            */
  int out_c;                   /* output (batch, out_h, out_w, out_c)          */
  int kernel_h, kernel_w;      /* out_h = (in_h + 2*pad - dilation*(kernel_h-1) - 1)/stride + 1 */
  int stride, pad, dilation;
} jtsm_conv_shape;

int jtsm_conv_out_size(const jtsm_conv_shape* s, int* out_h, int* out_w);
/* Bytes of scratch the forward (backward_data = 0) or backward-data (= 1) call of this shape can use
 * for deterministic split-K (layers with too few output tiles to fill 256 CUs are split along K into
 * per-slice slabs that a second kernel folds in slice order and finishes with the fused epilogue).
 * 0 = not split.  Passing a NULL / smaller workspace is allowed: the call then runs unsplit. */
size_t jtsm_conv_workspace_bytes(const jtsm_conv_shape* s, int backward_data);
/* Introspection for benchmarks/profiles: which kernel a call of this shape launches (kernel 0 =
 * register-staged igemm_kernel, 1 = double-buffered direct-to-LDS igemm_dma_kernel<..,2>, 2 = its
 * single-buffered form igemm_dma_kernel<..,1> used for short K sweeps), its tile and K-split.
 * role: 0 forward, 1 backward-data, 2 backward-weight. */
int jtsm_conv_plan(const jtsm_conv_shape* s, int role, int has_kscale, int* kernel, int* tile_m,
                   int* tile_n, int* splits);

/* y = relu?( conv(x, w) * scale[c] + bias[c] + residual ).  scale, bias, residual may be NULL;
 * residual has y's shape and may alias y. */
int jtsm_conv2d_forward_f32(const float* x, const float* w, float* y, const jtsm_conv_shape* s,
                            const float* scale, const float* bias, const float* residual,
                            int relu, void* workspace, size_t workspace_bytes, void* stream);
/* dx = conv_transpose(dy * kscale[out_c], w) (+ accumulate), then zeroed where
 * relu_mask <= 0.  kscale (per out_c; the FrozenBN scale of this conv), accumulate and
 * relu_mask (both dx-shaped; accumulate may alias dx) may be NULL. */
int jtsm_conv2d_backward_data_f32(const float* dy, const float* w, float* dx,
                                  const jtsm_conv_shape* s, const float* kscale,
                                  const float* accumulate, const float* relu_mask, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* dw[o][kh][kw][i] (+)= row_scale[o] * sum_pixels dy[p][o] * x[pix(p,kh,kw)][i].
 * zero_dw != 0 clears dw first; otherwise the result is added to what dw holds.  Split over
 * the pixel axis with float atomics: the last bits depend on arrival order. */
int jtsm_conv2d_backward_weight_f32(const float* dy, const float* x, float* dw,
                                    const jtsm_conv_shape* s, const float* row_scale, int zero_dw,
                                    void* stream);

/* Split-bf16 ("bf16x3") contractions: the same fp32-in / fp32-out convolution as above (same shapes,
 * epilogue, workspace and split-K rules), computed on the bf16 matrix cores from operands that were split
 * once into two bf16 planes, hi = bf16(x), lo = bf16(x - hi), as a_lo*b_hi + a_hi*b_lo + a_hi*b_hi with
 * fp32 accumulation (relative error per product ~2^-16; the reference is plain fp32 cuDNN/ATen conv,
 * detectron2/layers/wrappers.py:62-83).  Planes are raw bf16 bit patterns (uint16_t), 16-byte aligned.
 *   jtsm_split_bf16_f32             hi/lo[i] <- src[i], same layout (activations NHWC, weights OHWI)
 *   jtsm_split_bf16_transposed_f32  w [out_c][taps][in_c] -> planes of [in_c][taps][out_c] (what the
 *                                   data gradient contracts against); row_scale (nullable, [out_c])
 *                                   multiplies row o first — the FrozenBN scale of the layer
 *   jtsm_split_bf16_paired_f32      src [rows][k] (k % 32 == 0) -> PAIRED planes: per row, blocks of [32 k of hi]
 *                                   [32 k of lo], i.e. element (row, j) has hi at row*2k + (j/32)*64 + j%32 and lo 32
 *                                   elements behind it; `planes` holds 2*rows*k elements.  One K stage of a contraction
 *                                   (32 k of both planes) is then ONE whole 128-byte line per row instead of half a line
 *                                   of each of two arrays.  The WEIGHT operand (w_hi, w_lo / wt_hi, wt_lo) of every
 *                                   forward / backward-data plane entry point may be given in this layout (bf16x3): it is
 *                                   recognised by w_lo == w_hi + 32 elements (separate planes are at least a whole plane
 *                                   apart; keep them more than 32 elements apart).  jtsm_split_bf16_transposed_f32 and the
 *                                   records of jtsm_split_bf16_multi_f32 write paired planes when given such a pair
 *                                   (taps * out_c % 32 == 0; a straight record then carries its row length k in `in_c`)
 *   jtsm_conv_bf16x3_eligible       1 when a shape can take this path in `role` (0 forward, 1 backward-
 *                                   data; 2 see below): the contracted channel count is a multiple of 32, or the kernel
 *                                   is 1x1 and it is a multiple of 8 */
int jtsm_split_bf16_f32(const float* src, uint16_t* hi, uint16_t* lo, long n, void* stream);
int jtsm_split_bf16_paired_f32(const float* src, uint16_t* planes, long rows, int k, void* stream);
int jtsm_split_bf16_transposed_f32(const float* w, const float* row_scale, uint16_t* hi, uint16_t* lo,
                                   int out_c, int taps, int in_c, void* stream);
/* The same two splits for MANY weights in one launch.  table: device array of `entries` records of eight
 * 64-bit words {src, hi, lo, row_scale (transposed only, may be 0), first_block, n, taps, in_c}:
 *   transposed == 0: n = element count; the record owns ceil(n / 2048) consecutive workgroups;
 *   transposed != 0: n = out_c;          it owns ceil(in_c/32) * ceil(out_c/32) * taps workgroups.
 * first_block is the running sum of those counts (first record 0), `blocks` their total. */
int jtsm_split_bf16_multi_f32(const void* table, int entries, long blocks, int transposed, void* stream);
int jtsm_conv_bf16x3_eligible(const jtsm_conv_shape* s, int role);
/* What a bf16x3 call of this shape launches (given the advertised workspace): the template arguments of
 * igemm_x3_kernel<role,WM,WN,TM,TN,NBUF> (role 0/1) or igemm_x3_wgrad_kernel<WM,WN,TM,TN,NBUF> (role 2) —
 * WM x WN wavefronts of TM x TN 32x32 MFMA tiles — and the number of K slices.  *nbuf == 0 reports the LDS-halo
 * 3x3 kernel igemm_x3_halo_kernel<role,TH,WM,WN,TN,HP16> (TH = 8 * WM / 2 patch rows, HP16 = 12 or 21). */
int jtsm_conv_bf16x3_plan(const jtsm_conv_shape* s, int role, int* wm, int* wn, int* tm, int* tn, int* nbuf,
                          int* splits);

/* fp16 contractions (BASELINE.json configs[4]: "fp16 MFMA path" — fp16 operands, fp32 accumulate, fp32 results and
 * losses; the reference reaches fp16 through torch autocast, detectron2/engine/train_loop.py AMPTrainer).  Same
 * shapes, epilogue, workspace, eligibility and split-K rules as bf16x3, but every operand is ONE
 * plane of IEEE binary16 bit patterns (uint16_t, 16-byte aligned) and a product is one v_mfma_f32_32x32x16_f16.
 *   jtsm_split_f16_f32              h[i] <- fp16(src[i] * 2^shift), same layout
 *   jtsm_split_f16_transposed_f32   as jtsm_split_bf16_transposed_f32, one plane
 *   jtsm_split_bf16_multi_f32       with a record's `lo` word 0 writes that record's fp16 plane into `hi`
 * Activation and weight planes are plain fp16; gradient planes carry a power-of-two factor (grad_shift below). */
int jtsm_split_f16_f32(const float* src, uint16_t* h, long n, int shift, void* stream);
int jtsm_split_f16_transposed_f32(const float* w, const float* row_scale, uint16_t* h, int out_c, int taps, int in_c,
                                  void* stream);

/* ---- The plane entry points: ONE function per contraction role, for both plane arithmetics.
 * They compute what the _f32 entry points above compute (same shapes, epilogue, workspace and split-K rules;
 * eligibility: jtsm_conv_bf16x3_eligible) from operand planes.  The ARITHMETIC is told by the two input lo planes:
 * both given = bf16x3 (hi + lo per operand); both null = fp16, the *_hi arguments being the single fp16 planes.  One
 * given and one not is refused, and so is an option used against its line below ("fp16 only", "not together with",
 * "need"): JTSM_EINVAL with a jtsm_last_error text, nothing launched.  Every option is a nullable argument; null (0 for
 * grad_shift) = not wanted.
 *   output planes  y_hi, y_lo / dx_hi, dx_lo: planes of the FINISHED result (after the whole epilogue), written for a
 *                  following contraction — saves that layer's split pass; with a gate the dx planes ARE the layer
 *                  below's gated gradient, ready for its own two contractions.  bf16x3: both or neither.  fp16: the one
 *                  plane goes in *_hi and *_lo must be null; y's plane is plain, dx's carries 2^grad_shift again.  Need
 *                  the result's channel count % 4 == 0 and 16-byte aligned tensors; the strided 1x1 scatter form of the
 *                  data gradient produces none.
 *   fp32 result    y / dx may be NULL when its planes are requested: the fp32 copy is then never written (a chain that
 *                  keeps its activations as planes only: the mask heads' tower, layers/fused_blocks.py).
 *   gate_plane     the ReLU gate of relu_mask read from the gated activation's hi (bf16) or only (fp16) plane instead of
 *                  its fp32 copy (16-byte aligned, same layout as the result): the result is kept where the 16-bit pattern
 *                  is a positive number — the same gate (both formats round a positive fp32 to a positive value) at half
 *                  the bytes.
 *   row_scale      backward-data: one factor per result ROW (pixel or roi), applied first — the data gradient of a layer
 *                  whose input rows were rescaled, e.g. the per-roi factor in front of the box head
 *                  (projects/WSL/wsl/modeling/roi_heads/roi_heads_jtsm.py:607-633); needs in_c % 4 == 0.
 *                  backward-weight: one factor per out_c, as in jtsm_conv2d_backward_weight_f32.
 *   residual_h /   fp16 only (the reference's AMP step keeps activations and their gradients in fp16,
 *   accumulate_h   detectron2/engine/train_loop.py:289-336): the residual / the accumulate term read from an fp16 plane
 *                  — a block input that has no fp32 copy: y = relu?(conv * scale + bias + half(residual_h)); the shortcut
 *                  path's gradient, carrying 2^grad_shift: dx = conv^T(dy) + accumulate_h * 2^-grad_shift, then row
 *                  scale / gate_plane.  Not together with the fp32 twin (residual / accumulate); accumulate_h not with
 *                  relu_mask or colsum either.  Need out_c (in_c) % 4 == 0; not the strided 1x1 scatter.
 *   colsum         backward-data (also the transposed convolution's): ALSO leave the column sums of the finished, gated
 *                  result: rows x in_c floats, rows = jtsm_conv_bf16x3_colsum_rows(s, role) (role 0 for the transposed
 *                  convolution's conv shape, 1 for a data gradient; 0 rows: not available for this shape), one partial
 *                  sum per row tile of the launch, which the caller adds up in order (jtsm_colsum_fold_f32) — the bias
 *                  gradient of the layer below (ATen convolution_backward's grad_bias, detectron2/layers/wrappers.py:
 *                  76-78), taken where that layer's output gradient is written instead of by a pass over it (sums of the
 *                  fp32 values: no plane shift in them).  16-byte aligned.
 *   db             backward-weight: ALSO the bias gradient db[out_c] = sum over output pixels of dy (ATen
 *                  convolution_backward's third result / nn.Linear's bias gradient) in the same contraction: the
 *                  workgroups of the first column tile run one extra matrix instruction per dy fragment against an
 *                  all-ones fragment, so dy is not read a second time.  db comes from the same planes as dW.  Workspace:
 *                  jtsm_conv_bf16x3_wgrad_bias_workspace_bytes (the slabs of jtsm_conv_bf16x3_wgrad_workspace_bytes + the
 *                  bias partials).
 *   grad_shift     fp16 only (0 under bf16x3), 0..24: GRADIENT planes (dy, g, accumulate_h and the dx plane written) carry
 *                  the power-of-two factor 2^grad_shift (exact; keeps small gradients out of fp16's subnormal range — the
 *                  per-contraction equivalent of loss scaling): the caller splits dy with shift = grad_shift, the kernels
 *                  multiply the accumulator by 2^-grad_shift before the epilogue, so dx, dw and db come out unscaled, fp32.
 * backward-weight is eligible (role 2) when in_c and out_c are multiples of 8.  Unlike the fp32 kernel it is
 * DETERMINISTIC: each pixel slice writes a partial tile into the workspace (jtsm_conv_bf16x3_wgrad_workspace_bytes,
 * 16-byte aligned) and a fixed-order pass adds them; zero_dw == 0 adds the result to what dw holds. */
int jtsm_conv2d_forward_planes(const uint16_t* x_hi, const uint16_t* x_lo, const uint16_t* w_hi,
                               const uint16_t* w_lo, float* y, uint16_t* y_hi, uint16_t* y_lo,
                               const jtsm_conv_shape* s, const float* scale, const float* bias,
                               const float* residual, const uint16_t* residual_h, int relu, void* workspace,
                               size_t workspace_bytes, void* stream);
int jtsm_conv2d_backward_data_planes(const uint16_t* dy_hi, const uint16_t* dy_lo, const uint16_t* wt_hi,
                                     const uint16_t* wt_lo, float* dx, uint16_t* dx_hi, uint16_t* dx_lo,
                                     const jtsm_conv_shape* s, const float* row_scale, const float* accumulate,
                                     const uint16_t* accumulate_h, const float* relu_mask, const uint16_t* gate_plane,
                                     int grad_shift, float* colsum, void* workspace, size_t workspace_bytes,
                                     void* stream);
int jtsm_conv_bf16x3_colsum_rows(const jtsm_conv_shape* s, int role);
size_t jtsm_conv_bf16x3_wgrad_workspace_bytes(const jtsm_conv_shape* s);
size_t jtsm_conv_bf16x3_wgrad_bias_workspace_bytes(const jtsm_conv_shape* s);
int jtsm_conv2d_backward_weight_planes(const uint16_t* dy_hi, const uint16_t* dy_lo, const uint16_t* x_hi,
                                       const uint16_t* x_lo, float* dw, float* db, const jtsm_conv_shape* s,
                                       const float* row_scale, int zero_dw, int grad_shift, void* workspace,
                                       size_t workspace_bytes, void* stream);
/* Up to 8 weight gradients of ONE shape in a single launch (+ one finishing launch): member i is
 * dw[i] = row_scale[i][out] * sum_pixels dy_i (x) x_i (fresh results; row_scale may be NULL, or hold NULL members).
 * dy_hi .. x_lo are HOST arrays of n device pointers; the arithmetic is told by the two lo ARRAYS (both null: fp16).
 * For the layers a network repeats (the bottleneck blocks of a ResNet stage: same ATen convolution_backward, weight
 * output only, as jtsm_conv2d_backward_weight_planes): the K (pixel) axis of the whole group is cut into as many slices
 * as ONE launch needs to fill the chip — a sixth of the slabs six separate launches write and fold.  Deterministic (slabs
 * folded in slice order); results are bit-identical for a given (shape, n), not to the single-layer entry (different
 * slicing).  Workspace: jtsm_conv_bf16x3_wgrad_group_workspace_bytes(s, n); jtsm_conv_bf16x3_wgrad_group_plan reports
 * the kernel (tile: 0 = the 3x3 LDS-halo kernel, 128, 256) and the slice count. */
size_t jtsm_conv_bf16x3_wgrad_group_workspace_bytes(const jtsm_conv_shape* s, int n);
int jtsm_conv_bf16x3_wgrad_group_plan(const jtsm_conv_shape* s, int n, int* tile, int* splits);
int jtsm_conv2d_backward_weight_group_planes(int n, const uint16_t* const* dy_hi, const uint16_t* const* dy_lo,
                                             const uint16_t* const* x_hi, const uint16_t* const* x_lo,
                                             float* const* dw, const float* const* row_scale,
                                             const jtsm_conv_shape* s, int grad_shift, void* workspace,
                                             size_t workspace_bytes, void* stream);
/* ---- ConvTranspose2d(kernel 2, stride 2, padding 0, bias) — the mask heads' upsampler
 * (detectron2/modeling/roi_heads/mask_head.py:245-252 `deconv`; projects/WSL/wsl/modeling/roi_heads/mask_head.py:303-305;
 * ATen conv_transpose2d behind detectron2/layers/wrappers.py `ConvTranspose2d = torch.nn.ConvTranspose2d`).
 * Tensors are NHWC: x (batch, h, w, in_c), y (batch, 2h, 2w, out_c); the weight is the parameter (in_c, out_c, 2, 2)
 * in channels_last memory order [in_c][dy][dx][out_c].  in_c % 32 == 0, out_c % 32 == 0.
 *   forward        y[b,2i+dy,2j+dx,o] = relu?(bias[o] + sum_c x[b,i,j,c] W[c][dy][dx][o]) — one GEMM whose epilogue
 *                  writes straight to the four output pixels.  wt_* = planes of W^T as
 *                  jtsm_split_bf16_transposed_f32(W, null, .., out_c = in_c, taps = 1, in_c = 4*out_c) makes them.
 *   backward_data  dx[b,i,j,c] = sum_{dy,dx,o} g[b,2i+dy,2j+dx,o] W[c][dy][dx][o], kept where relu_mask > 0 (nullable:
 *                  the ReLU output x came from) — the forward role of the 2x2/stride-2 convolution whose OHWI weight is
 *                  the same memory: w_* = plain planes of W (jtsm_split_bf16_f32);
 *                  workspace: jtsm_conv_transpose2x2_workspace_bytes (may be null: no K split).
 *   backward_weight: jtsm_conv2d_backward_weight_planes with shape {batch, 2h, 2w, in_c = out_c, out_c = in_c, 2, 2,
 *                  stride 2, pad 0}, dy planes = x's, x planes = g's: dW comes out in the parameter's memory order.
 * Arithmetic, output planes (y_hi, y_lo / dx_hi, dx_lo), null fp32 result, gate_plane, colsum and grad_shift (g's
 * planes carry it) as described for the plane entry points above. */
int jtsm_conv_transpose2x2_forward_planes(const uint16_t* x_hi, const uint16_t* x_lo, const uint16_t* wt_hi,
                                          const uint16_t* wt_lo, float* y, uint16_t* y_hi, uint16_t* y_lo, int batch,
                                          int h, int w, int in_c, int out_c, const float* bias, int relu, void* stream);
size_t jtsm_conv_transpose2x2_workspace_bytes(int batch, int h, int w, int in_c, int out_c);
int jtsm_conv_transpose2x2_backward_data_planes(const uint16_t* g_hi, const uint16_t* g_lo, const uint16_t* w_hi,
                                                const uint16_t* w_lo, float* dx, uint16_t* dx_hi, uint16_t* dx_lo,
                                                int batch, int h, int w, int in_c, int out_c, const float* relu_mask,
                                                const uint16_t* gate_plane, int grad_shift, float* colsum,
                                                void* workspace, size_t workspace_bytes, void* stream);
/* Streaming passes that end in operand planes (hi + lo bf16, or lo == NULL: one fp16 plane of v * 2^shift; all
 * pointers 16-byte aligned, element counts multiples of 8):
 *   jtsm_relu_backward_split_scaled_f32  g = y > 0 ? dy * scale : 0 (+ planes of g): the backward of ReLU followed by
 *       inverted dropout when y is the DROPOUT's output (positive exactly where the unit was kept and active;
 *       scale = 1 / (1 - p)) — torch.nn.functional.dropout + F.relu of the box head,
 *       projects/WSL/wsl/modeling/roi_heads/box_head.py DiscriminativeAdaptionNeck;
 *   jtsm_split_rowscale_f32              planes of src[r][c] * row_scale[r] (nothing else is written): the per-roi
 *       rescale in front of the box head (roi_heads_jtsm.py:607-633) folded into the plane split;
 *   jtsm_dropout_split_f32               y = keep(i) ? x / (1 - p) : 0 (y may alias x) + planes of y (y_hi nullable);
 *       keep(i) is a counter-based hash of (seed, i), so no mask is stored;
 *   jtsm_channel_sum_planes              the bias gradient (jtsm_channel_sum_ws_f32) of a gradient held as planes:
 *       out[c] = sum_r (hi + lo)[r][c] (lo null: the fp16 plane times 2^-shift); C % 8 == 0; workspace of 1024 * C
 *       floats. */
int jtsm_relu_backward_split_scaled_f32(const float* dy, const float* y, float scale, float* g, uint16_t* g_hi,
                                        uint16_t* g_lo, long n, int shift, void* stream);
int jtsm_split_rowscale_f32(const float* src, const float* row_scale, long rows, int cols, uint16_t* hi, uint16_t* lo,
                            int shift, void* stream);
int jtsm_dropout_split_f32(const float* x, float* y, uint16_t* y_hi, uint16_t* y_lo, long n, float p,
                           unsigned long long seed, void* stream);
int jtsm_channel_sum_planes(const uint16_t* hi, const uint16_t* lo, float* out, long rows, int C, int shift,
                            void* workspace, size_t workspace_bytes, void* stream);
/* Up to 8 such gradients of one width C in a single launch (+ one fold): hi[i] / lo[i] (lo NULL: fp16 planes) with
 * rows[i] rows each -> outs[i][C]; workspace of count * 1024 * C floats. */
int jtsm_channel_sum_planes_multi(const uint16_t* const* hi, const uint16_t* const* lo, float* const* outs,
                                  const long* rows, int count, int C, int shift, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* g = dy where y > 0 else 0 (fp32), and g's fp16 plane times 2^shift (n % 8 == 0) in the same pass. */
int jtsm_relu_backward_split_f16(const float* dy, const float* y, float* g, uint16_t* g_h, long n, int shift,
                                 void* stream);

/* ---------------------------------------------------------------------------
 * Bandwidth-bound helpers (no reference source: torch elementwise ops behind
 * F.relu_ / autograd, e.g. detectron2/modeling/backbone/resnet.py:196-210).
 * ------------------------------------------------------------------------- */
/* g[i] = y[i] > 0 ? dy[i] : 0   (y = the ReLU's output). */
/* g = dy where y > 0 else 0, and the bf16 hi / lo planes of g (n % 8 == 0) in the same pass. */
int jtsm_relu_backward_split_f32(const float* dy, const float* y, float* g, uint16_t* g_hi, uint16_t* g_lo,
                                 long n, void* stream);
int jtsm_relu_backward_f32(const float* dy, const float* y, float* g, long n, void* stream);
/* out[c] = sum_r g[r*C + c]  — bias gradient of a conv / linear layer. */
int jtsm_channel_sum_f32(const float* g, float* out, long rows, int C, void* stream);
/* The same for n <= 16 small (rows[b] x width) matrices in one launch, rows added in order: out (n, width) — folds the
 * per-row-tile column sums (`colsum` of the plane entry points' data gradients) of several layers at once. */
int jtsm_colsum_fold_f32(const float* const* parts, const int* rows, int n, int width, float* out, void* stream);
/* The same without atomics (bitwise reproducible) and ~4x faster on large inputs: row slabs are summed into
 * `workspace` (jtsm_channel_sum_workspace_bytes, 16-byte aligned) and folded in slab order, for any C and any
 * number of rows.  Falls back to the (atomic) form above only when the workspace is missing or too small. */
size_t jtsm_channel_sum_workspace_bytes(long rows, int C);
int jtsm_channel_sum_ws_f32(const float* g, float* out, long rows, int C, void* workspace, size_t workspace_bytes,
                            void* stream);
/* SGD with momentum over many tensors in ONE launch — torch.optim.SGD as detectron2/solver/build.py:110-195
 * configures it (dampening 0, no nesterov): d = g + wd*p; buf = first_step ? d : mu*buf + d; p -= lr*buf.
 * table: device array of `entries` records of eight 64-bit words {param, grad, momentum_buffer, n, first_block,
 * lr, weight_decay, momentum} (the three floats as their bit patterns in the low 32 bits); a record owns
 * ceil(n / 1024) consecutive workgroups, first_block is the running sum, `blocks` the total. */
int jtsm_sgd_momentum_multi_f32(const void* table, int entries, long blocks, int first_step, void* stream);


/* NHWC spatial helpers, C % 4 == 0 (no reference source; torch ops at
 * detectron2/modeling/backbone/resnet.py:358 (max_pool2d 3,2,1), fpn.py:133-136
 * (interpolate nearest x2 + add), fpn.py:173-185 (max_pool2d 1,2,0)). */
int jtsm_maxpool3x3s2_forward_f32(const float* x, float* y, int N, int H, int W, int C, void* stream);
/* Every element of gx is written; the gradient goes to the first maximum of each window, gathered per input pixel over
 * the <= 2 x 2 windows that hold it, in window order (no float atomics: the same bits on every run). */
int jtsm_maxpool3x3s2_backward_f32(const float* x, const float* gy, float* gx, int N, int H, int W,
                                   int C, void* stream);
/* 2x2 max pooling of the WSL ResNet-v2 backbone (projects/WSL/wsl/modeling/backbone/resnet_wsl_v2.py:157-165,413):
 * stride 2 = MaxPool2d(2, 2) -> (N, H/2, W/2, C); stride 1 = ZeroPad2d((0,1,0,1)) + MaxPool2d(2, 1) -> (N,H,W,C).
 * NHWC; backward is a gather (first maximum of a window wins, as ATen). */
int jtsm_maxpool2x2_forward_f32(const float* x, float* y, int N, int H, int W, int C, int stride, void* stream);
int jtsm_maxpool2x2_backward_f32(const float* x, const float* gy, float* gx, int N, int H, int W, int C,
                                 int stride, void* stream);
/* out(N,H,W,C) = lateral(N,H,W,C) + top(N,H/2,W/2,C) repeated 2x2. */
int jtsm_upsample2_add_f32(const float* top, const float* lateral, float* out, uint16_t* out_hi, uint16_t* out_lo,
                           int N, int H, int W, int C, void* stream);   /* out_hi / out_lo (optional): bf16 planes of out */
/* out = inputs[0] + inputs[1] (+ ...), n <= 4 dense tensors of `numel` floats summed in list order (HOST array of
 * device pointers), optional bf16 planes of the sum: the level sum of SemSegFPNHead.layers
 * (detectron2/modeling/meta_arch/semantic_seg.py:178-186) in one pass. */
int jtsm_sum_tensors_f32(const float* const* inputs, int n, long numel, float* out, uint16_t* out_hi, uint16_t* out_lo,
                         void* stream);
/* out(N,Ht,Wt,C) = sum over the 2x2 blocks of g(N,2Ht,2Wt,C): backward of the x2 upsample. */
int jtsm_sum2x2_f32(const float* g, float* out, int N, int Ht, int Wt, int C, void* stream);
/* scatter=0: dst(N,Ho,Wo,C) = src(N,H,W,C)[:, ::2, ::2]; scatter=1: dst(N,H,W,C) zero-filled, then
 * dst[:, ::2, ::2] = src(N,Ho,Wo,C).  Ho = (H-1)/2+1. */
int jtsm_subsample2_f32(const float* src, float* dst, int N, int H, int W, int C, int scatter,
                        void* stream);


/* ---------------------------------------------------------------------------
 * Multiple-instance-learning losses of projects/WSL, fused forward + analytic backward.
 * No native reference: they replace PyTorch arithmetic at
 *   fast_rcnn_tsm.py:573-586 (scores = softmax(C,1) * per-image softmax(D,0)),
 *   :840-854 / :346-379 (image probabilities = clamp(sum over the image's proposals), BCE)
 *   fast_rcnn_oicr.py:282-298 (weighted CE / #valid), :350-380 (weighted L1 on the gt-class
 *   deltas / R, Box2BoxTransform weights (10,10,5,5), detectron2/modeling/box_regression.py:38-71)
 * (all under projects/WSL/wsl/modeling/roi_heads/).  Rows of image i are
 * [bag_offsets[i], bag_offsets[i+1]).  Logit matrices are row-major with leading dimension
 * `ld*` (columns of a wider fused predictor output are fine).  nc, num_cls <= 192.
 * ------------------------------------------------------------------------- */
size_t jtsm_mil_workspace_bytes(int nbags, int max_bag_rows, int nc);
/* scores (R,nc) dense; img_probs (nbags,nc) clamped to [1e-6, 1-1e-6]; loss: 1 float
 * (mean over nbags*nc when mean_loss, else sum/nbags).  labels (nbags,nc) float 0/1.
 * The workspace keeps what the backward needs and must stay untouched until then. */
int jtsm_mil_forward_f32(const float* cls_logits, const float* det_logits, int ld, int nc,
                         const int32_t* bag_offsets, int nbags, int max_bag_rows,
                         const float* labels, int mean_loss, float* scores, float* img_probs,
                         float* loss, void* workspace, void* stream);
/* d_cls/d_det (R, nc) with leading dimension ld_grad = upstream[0] * dloss/dlogits
 * (upstream NULL = 1). */
int jtsm_mil_backward_f32(const float* cls_logits, const float* det_logits, int ld, int nc,
                          const int32_t* bag_offsets, int nbags, int max_bag_rows,
                          const float* upstream, float* d_cls, float* d_det, int ld_grad,
                          const void* workspace, void* stream);

size_t jtsm_oicr_workspace_bytes(void);
/* labels (R) int32 in [-1, num_cls-1] (num_cls-1 = background, -1 = ignored); weights (R);
 * proposals / gt_boxes (R,4) xyxy.  box_deltas (R, 4*(num_cls-1)) may be NULL (no box branch).
 * losses[0] = loss_cls, losses[1] = loss_box_reg, losses[2] = #rows with weight > 1e-12. */
int jtsm_oicr_forward_f32(const float* cls_logits, int ld_cls, int num_cls, const float* box_deltas,
                          int ld_box, const int32_t* labels, const float* weights,
                          const float* proposals, const float* gt_boxes, int R, float* losses,
                          void* workspace, void* stream);
/* d_cls (R,num_cls) with leading dimension ld_dcls, d_box (R,4*(num_cls-1)) with ld_dbox (may be NULL);
 * up_cls / up_box: device scalars (NULL = 1); `losses` is the forward's output. */
int jtsm_oicr_backward_f32(const float* cls_logits, int ld_cls, int num_cls, const float* box_deltas,
                           int ld_box, const int32_t* labels, const float* weights,
                           const float* proposals, const float* gt_boxes, int R, const float* losses,
                           const float* up_cls, const float* up_box, float* d_cls, int ld_dcls,
                           float* d_box, int ld_dbox, void* stream);

/* The same two with detectron2's smooth_l1_loss(beta) (MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA) in the box term: per
 * component n = |d - t|, 0.5 n^2 / beta where n < beta, n - 0.5 beta elsewhere; beta < 1e-5 is L1 and computes exactly
 * what jtsm_oicr_forward_f32 / jtsm_oicr_backward_f32 compute.  Same workspace. */
int jtsm_oicr_smooth_forward_f32(const float* cls_logits, int ld_cls, int num_cls, const float* box_deltas,
                                 int ld_box, const int32_t* labels, const float* weights,
                                 const float* proposals, const float* gt_boxes, int R, float beta,
                                 float* losses, void* workspace, void* stream);
int jtsm_oicr_smooth_backward_f32(const float* cls_logits, int ld_cls, int num_cls, const float* box_deltas,
                                  int ld_box, const int32_t* labels, const float* weights,
                                  const float* proposals, const float* gt_boxes, int R, float beta,
                                  const float* losses, const float* up_cls, const float* up_box, float* d_cls,
                                  int ld_dcls, float* d_box, int ld_dbox, void* stream);


/* ---------------------------------------------------------------------------
 * PCL — proposal clustering and the PCL loss of one refinement branch, for all images at once.
 * Replaces PCL() (projects/WSL/wsl/modeling/roi_heads/third_party/pcl.py:24-200: numpy and
 * scikit-learn on the host) and pcl_loss_forward / pcl_loss_backward
 * (projects/WSL/wsl/layers/csrc/pcl_loss/pcl_loss.h:9-131; the CPU kernels pcl_loss_cpu.cpp:8-115
 * are the ones wsl/layers/pcl_loss.py:9-93 reaches).  Contract spelled out in jtsm_amd/csrc/pcl.hip;
 * k-means is a declared deterministic substitution.
 * Rows of image i are [offsets[i], offsets[i+1]); max_rows bounds the rows of one image (<= 8192).
 * boxes (R,4) xyxy, 16-byte aligned.  prev_probs: the previous branch's probabilities, class c in
 * column prev_col0 + c.  labels (nimg,K) float 0/1.  probs (R,K+1): this branch's soft-max,
 * background in column 0.  Outputs: row_label (R) in [0,K] (0 = background), row_assign (R)
 * cluster index or -1, row_weight (R); per image 5K cluster slots: pc_int (nimg,5K,3) =
 * (label, member count, centre row), pc_flt (nimg,5K,3) = (centre score, summed member weight,
 * pc_prob); pc_num (nimg) clusters used.  No float atomics: the same inputs give the same tables.
 * ------------------------------------------------------------------------- */
size_t jtsm_pcl_cluster_workspace_bytes(int nimg, int max_rows);
int jtsm_pcl_cluster_f32(const float* boxes, const int32_t* offsets, int nimg, int max_rows, int total_rows,
                         const float* prev_probs, int ld_prev, int prev_col0, const float* labels,
                         int num_classes, const float* probs, int ld_probs, int32_t* row_label,
                         int32_t* row_assign, float* row_weight, int32_t* pc_int, float* pc_flt,
                         int32_t* pc_num, void* workspace, void* stream);
/* probs (R,num_cls) dense = softmax over the num_cls columns of logits (leading dimension ld). */
int jtsm_pcl_softmax_f32(const float* logits, int ld, int num_cls, int R, float* probs, void* stream);
size_t jtsm_pcl_loss_workspace_bytes(int nimg);
/* loss[0] = mean over the images of (background term + cluster term) / rows of the image. */
int jtsm_pcl_loss_forward_f32(const float* probs, int ld_probs, const int32_t* offsets, int nimg,
                              int num_classes, const int32_t* row_label, const float* row_weight,
                              const int32_t* pc_int, const float* pc_flt, const int32_t* pc_num,
                              float* loss, void* workspace, void* stream);
/* d_logits (R,K+1) with leading dimension ld_grad = upstream[0] * dloss/dlogits (upstream NULL = 1;
 * the reference ignores the upstream gradient, pcl_loss.py:55-90), soft-max backward included. */
int jtsm_pcl_loss_backward_f32(const float* logits, int ld, int num_classes, const int32_t* offsets,
                               int nimg, int total_rows, const int32_t* row_label,
                               const int32_t* row_assign, const float* row_weight, const int32_t* pc_int,
                               const float* pc_flt, const float* upstream, float* d_logits, int ld_grad,
                               void* stream);


/* Mask targets of rectangle pseudo ground truth (get_pgt_mask, roi_heads_jtsm.py:1928-1994, with the rectangle
 * substitution of SURVEY F8; BitMasks.crop_and_resize, detectron2/structures/masks.py:169-200):
 * out[n] (side x side, 0/1 bytes) = ROIAlign(1.0, sampling_ratio 0, aligned) of the H x W bitmask "pixel centre
 * inside rects[n] shrunk by erode" over rois[n], thresholded at 0.5.  rois, rects: (N,4) boxes.  The bitmask is
 * never materialised; the sampling arithmetic is that of jtsm_roi_align_forward_f32. */
int jtsm_rect_mask_targets_f32(const float* rois, const float* rects, uint8_t* out, int N, int side, int H, int W,
                               float erode, void* stream);
/* Mask targets from superpixel evidence (object_evidence, projects/WSL/wsl/modeling/roi_heads/roi_heads_jtsm.py:
 * 1928-1994): target n is the union of the superpixels that row oh_row[n] of oh_labels (R, L) int32 marks, in image
 * img_of[n] of superpixels (B, H, W) int32, cropped to rois[n] at side x side as BitMasks.crop_and_resize does
 * (detectron2/structures/masks.py:169-200) and thresholded at 0.5.  oh_row[n] < 0 gives an all-zero target. */
int jtsm_sp_mask_targets_f32(const float* rois, const int32_t* oh_row, const int32_t* img_of, const int32_t* oh_labels,
                             int L, const int32_t* superpixels, uint8_t* out, int N, int side, int H, int W,
                             void* stream);
/* Targets of the mask refinery (get_pgt_mask, roi_heads_jtsm.py:1997-2022): probs (N, M, M) pasted into the H x W
 * image at rois[n] (paste_masks_in_image, detectron2/layers/mask_ops.py:74-152, >= threshold) and cropped back to
 * the same box at side x side (crop_and_resize, >= 0.5), without storing the pasted image. */
int jtsm_paste_crop_targets_f32(const float* probs, const float* rois, uint8_t* out, int N, int M, int side, int H,
                                int W, float threshold, void* stream);
/* The "top_k nearest" targets of the mask branch (roi_heads_jtsm.py:840-905): near_rows (B, Gmax, top_k) int32 = for
 * every pseudo box the top_k foreground proposals (labels != bg_label) of its image by IoU, descending, ties by row,
 * -1 padded; matched_near (R) int32 = for every foreground proposal the near target (a proposal row) with the
 * highest IoU, first maximum in (pseudo box, rank) order; -1 for the others. */
int jtsm_near_targets_f32(const float* proposals, const int32_t* bag_offsets, int B, int R, const int32_t* labels,
                          int bg_label, const float* pgt_box, const int32_t* counts, int Gmax, int top_k,
                          int32_t* near_rows, int32_t* matched_near, void* stream);

/* Label preparation (no arithmetic of the model: the index / presence glue around it, which the reference writes as
 * dozens of small tensor ops).  Per-image inputs are B <= 16 device pointers with their row counts (host arrays).
 *
 * jtsm_pooler_rois_levels_f32 — ROIPooler's two helpers as one pass (detectron2/modeling/poolers.py:22-58
 *   assign_boxes_to_levels, :68-95 convert_boxes_to_pooler_format; projects/WSL/wsl/modeling/poolers.py:24-109):
 *   rois (M,5) = [image index, x0, y0, x1, y1]; level (M) = floor(canonical_level + log2(sqrt(area) /
 *   canonical_box_size + 1e-8)) clamped to [min_level, max_level], minus min_level (NaN -> 0).  Float operations in
 *   PyTorch's order (its division by a host scalar multiplies by the rounded reciprocal): same levels, bit for bit.
 * jtsm_roi_scale_f32 — the box head's per-roi factor (projects/WSL/wsl/modeling/roi_heads/roi_heads_jtsm.py:607-633):
 *   out[m] = bins / (nvalid[m] + 1) * (objectness[m] + 1), nvalid = bins of roi m whose MOIPool argmax (channel 0) is
 *   not -1; argmax (M, bins, C) int32 channels-last.
 * jtsm_image_labels — image-level labels (projects/WSL/wsl/modeling/roi_heads/roi_heads.py:146-161 get_image_level_gt,
 *   roi_heads_jtsm.py get_image_level_gt_stuff): oh_things (B, num_classes) 0/1 from each image's gt_classes (int64),
 *   things_cls (B, num_classes) = the present classes ascending, then the absent ones ascending; things_cnt (B) = how
 *   many are present.  With sem_seg (B x pixels labels of sem_elem_bytes 8 (int64) or 1 (uint8), clamped to 0..255):
 *   the same for the stuff labels 1 .. num_stuff - 1 (0 = things, 255 = ignore), columns label - 1, list entries
 *   column + stuff_offset.  workspace: jtsm_image_labels_workspace_bytes(B). */
int jtsm_pooler_rois_levels_f32(const float* const* boxes, const int* counts, int B, int min_level, int max_level,
                                float canonical_box_size, float canonical_level, float* rois, int32_t* level,
                                void* stream);
int jtsm_roi_scale_f32(const int32_t* argmax, int bins, int C, const float* const* objectness, const int* counts, int B,
                       float* out, void* stream);
size_t jtsm_image_labels_workspace_bytes(int B);
int jtsm_image_labels(const int64_t* const* gt_classes, const int* counts, int B, int num_classes, const void* sem_seg,
                      int sem_elem_bytes, long pixels, int num_stuff, int stuff_offset, float* oh_things,
                      int32_t* things_cls, int32_t* things_cnt, float* oh_stuff, int32_t* stuff_cls, int32_t* stuff_cnt,
                      void* workspace, void* stream);

/* The foreground proposals of the mask branch (projects/WSL/wsl/modeling/roi_heads/roi_heads_jtsm.py:754-948:
 * `select_foreground_proposals` + the gathers that follow it): rows with labels[r] != bg_label, in row order, with
 * their box, class (int64), image, matched near target (matched nullable) and (image, box) roi; counts[b] (int64) =
 * foreground rows of image b.  The fg_* buffers hold R entries, of which the first sum(counts) are written. */
int jtsm_fg_compact(const int32_t* labels, int bg_label, const int32_t* bag_offsets, int B, int R, const float* boxes,
                    const int32_t* matched, int32_t* fg_rows, float* fg_boxes, int64_t* fg_classes, int32_t* fg_img,
                    int32_t* fg_matched, float* fg_rois, int64_t* counts, void* stream);

/* Mask loss — mask_rcnn_loss (detectron2/modeling/roi_heads/mask_head.py:31-112, used by
 * projects/WSL/wsl/modeling/roi_heads/mask_head.py): mean binary cross-entropy with logits between the
 * ground-truth-class channel of logits (N,side,side,ld) NHWC (num_classes <= ld; gt_classes NULL when
 * class-agnostic, num_classes == 1) and target (N,side,side) 0/1 bytes.  out[0] = loss.  The backward writes the
 * dense dlogits (zero off the class channel).  Deterministic (fixed-order two-stage sum). */
size_t jtsm_mask_bce_workspace_bytes(void);
int jtsm_mask_bce_forward_f32(const float* logits, int ld, int num_classes, const int64_t* gt_classes,
                              const uint8_t* target, int N, int side, float* out, void* workspace,
                              void* stream);
int jtsm_mask_bce_backward_f32(const float* logits, int ld, int num_classes, const int64_t* gt_classes,
                               const uint8_t* target, int N, int side, const float* upstream,
                               float* dlogits, void* stream);


/* ---------------------------------------------------------------------------
 * FPN-level variants (NHWC only) — what ROIPooler.forward does with nonzero + index +
 * scatter per level (detectron2/modeling/poolers.py:236-247,
 * projects/WSL/wsl/modeling/poolers.py:300-320), without the host synchronisation: every
 * level's launch walks ALL M rois and serves only those with roi_level[m] == level, reading
 * that level's feature map and writing rows m of the shared (M,PH,PW,C) output /
 * scattering rows m of the shared gradient into that level's grad_input (zero-filled by the
 * call).  Rows of other levels are left untouched.
 * ------------------------------------------------------------------------- */
int jtsm_roi_align_forward_level_f32(const float* input, const float* rois,
                                     const int32_t* roi_level, int level, float* output, int B,
                                     int C, int H, int W, int M, float spatial_scale, int pooled_h,
                                     int pooled_w, int sampling_ratio, int aligned, void* stream);
int jtsm_roi_align_backward_level_f32(const float* grad, const float* rois,
                                      const int32_t* roi_level, int level, float* grad_input, int B,
                                      int C, int H, int W, int M, float spatial_scale, int pooled_h,
                                      int pooled_w, int sampling_ratio, int aligned, void* stream);
/* Rotated boxes (M,6) on one FPN level: ROIPooler's level loop with pooler_type "ROIAlignRotated"
 * (detectron2/modeling/poolers.py:160-165,230-249; ROIAlignRotated.h:7-27 per level).  accumulate != 0: grad_input
 * already holds a gradient and is added to (nothing is cleared). */
int jtsm_roi_align_rotated_forward_level_f32(const float* input, const float* rois, const int32_t* roi_level,
                                             int level, float* output, int B, int C, int H, int W, int M,
                                             float spatial_scale, int pooled_h, int pooled_w, int sampling_ratio,
                                             void* stream);
int jtsm_roi_align_rotated_backward_level_f32(const float* grad, const float* rois, const int32_t* roi_level,
                                              int level, float* grad_input, int B, int C, int H, int W, int M,
                                              float spatial_scale, int pooled_h, int pooled_w, int sampling_ratio,
                                              int accumulate, void* stream);
/* All levels' gradient maps in ONE call (the backward of ROIPooler's level loop, detectron2/modeling/poolers.py:236-247):
 * grad_inputs[l] (nullable: that level needs no gradient) is the (B,H[l],W[l],C) NHWC map of the rois with
 * roi_level[m] == l.  The tiles of every level are workgroups of one launch.
 * accumulate != 0 (here and in jtsm_moi_pool_backward_levels_f32): the maps already hold a gradient — what autograd
 * would add afterwards, another consumer's term — and this call adds to it in place (nothing is cleared; every cell's
 * read-add-write belongs to one thread, still no atomics in the gather forms, still reproducible).
 * workspace: jtsm_roi_align_backward_levels_workspace_bytes(H, W, nlevels, B, C, M) bytes of caller-owned device memory,
 * 16-byte aligned (tile census, launch plan, per-roi reach tables) — no allocation inside the library; NULL makes the
 * call take stream-ordered scratch of its own. */
size_t jtsm_roi_align_backward_levels_workspace_bytes(const int* H, const int* W, int nlevels, int B, int C, int M);
int jtsm_roi_align_backward_levels_f32(const float* grad, const float* rois, const int32_t* roi_level,
                                       float* const* grad_inputs, const int* H, const int* W, const float* scales,
                                       int nlevels, int B, int C, int M, int pooled_h, int pooled_w, int sampling_ratio,
                                       int aligned, int accumulate, void* workspace, size_t workspace_bytes,
                                       void* stream);


/* ---------------------------------------------------------------------------
 * SemSegFPNHead's non-GEMM layers, NHWC (no reference source: nn.GroupNorm(32, C) applied by
 * Conv2d.forward, detectron2/layers/wrappers.py:79-82, and nn.Upsample(scale_factor=2, "bilinear",
 * align_corners=False), detectron2/modeling/meta_arch/semantic_seg.py:126-150).
 * group_norm: x,y (N, HW, C) with C/G a multiple of 4 and C/4 dividing 256; ReLU optionally folded in
 * (relu != 0: y = max(.,0), and the backward gates dy by the recomputed sign).  mean/rstd: (N,G) outputs
 * of the forward, inputs of the backward.  Reductions are two-stage in a fixed order (deterministic).
 * ------------------------------------------------------------------------- */
size_t jtsm_group_norm_workspace_bytes(int N, long HW, int C);
int jtsm_group_norm_forward_f32(const float* x, const float* gamma, const float* beta, float* y,
                                float* mean, float* rstd, void* workspace, int N, long HW, int C, int G,
                                float eps, int relu, void* stream);
/* dx_hi / dx_lo, y_hi / y_lo below (both or neither, nullable): bf16 planes of the result for a following
 * bf16x3 contraction (see jtsm_split_bf16_f32). */
int jtsm_group_norm_backward_f32(const float* x, const float* dy, const float* gamma, const float* beta,
                                 const float* mean, const float* rstd, float* dx, uint16_t* dx_hi,
                                 uint16_t* dx_lo, float* dgamma, float* dbeta, void* workspace, int N, long HW,
                                 int C, int G, int relu, void* stream);
/* y (N,2H,2W,C) <- x (N,H,W,C); backward is a gather (no atomics). */
int jtsm_upsample_bilinear2x_forward_f32(const float* x, float* y, uint16_t* y_hi, uint16_t* y_lo, int N, int H,
                                         int W, int C, void* stream);
int jtsm_upsample_bilinear2x_backward_f32(const float* gy, float* gx, int N, int H, int W, int C,
                                          void* stream);


/* The same up-sampling for any integer scale S >= 1 (the DeepLab v3+ decoder's F.interpolate(y, size=..., mode=
 * "bilinear", align_corners=False), projects/DeepLab/deeplab/semantic_seg.py:248, from stride 16 to stride 4):
 * y (N,S*H,S*W,C) <- x (N,H,W,C), C % 4 == 0, ATen's association of the four taps; the backward is a gather over the
 * <= 2S x 2S outputs that sample a source pixel (no atomics: the same bits on every run). */
int jtsm_upsample_bilinear_forward_f32(const float* x, float* y, int N, int H, int W, int C, int S, void* stream);
int jtsm_upsample_bilinear_backward_f32(const float* gy, float* gx, int N, int H, int W, int C, int S, void* stream);

/* Fused "bilinear xS up-sampling (align_corners=False) + cross_entropy(mean, ignore_index)" of
 * SemSegFPNHead.losses (detectron2/modeling/meta_arch/semantic_seg.py:179-188): the full-resolution
 * logits are never materialised.  logits: (N,Hs,Ws,ld) NHWC, 16-byte aligned, with C <= ld <= 64 classes and
 * ld % 4 == 0 (ld = channel pitch: a 56-wide map holding 54 classes); target: (N,Hs*S,Ws*S) int64.
 * out[0] = loss, out[1] = number of non-ignored pixels.  The workspace keeps one log-sum-exp per output
 * pixel for the backward, which gathers (no atomics) and writes dlogits (N,Hs,Ws,ld), pad lanes zero. */
size_t jtsm_semseg_ce_workspace_bytes(int N, int Hs, int Ws, int S);
int jtsm_semseg_ce_forward_f32(const float* logits, int ld, int C, const int64_t* target, float* out,
                               void* workspace, int N, int Hs, int Ws, int S, long ignore_index,
                               void* stream);
int jtsm_semseg_ce_backward_f32(const float* logits, int ld, int C, const int64_t* target,
                                const float* fwd_out, const float* upstream, float* dlogits,
                                const void* workspace, int N, int Hs, int Ws, int S, long ignore_index,
                                void* stream);

/* ---------------------------------------------------------------------------
 * Trainable batch norm behind a convolution (replaces torch.nn.BatchNorm2d / nn.SyncBatchNorm / NaiveSyncBatchNorm as
 * get_norm hands them out, detectron2/layers/batch_norm.py:128-153, applied by Conv2d.forward, wrappers.py:79-82, and
 * the bottleneck's `out += shortcut; relu`, resnet.py:203-210).  Maps are channels-last fp32: R = N*H*W rows of C
 * channels; x has a leading dimension ld >= C (a [:, :C] slice of a wider map), every other map is dense.  float4
 * accesses are used where C, ld and the pointers allow, scalar ones otherwise: any C works.
 *   stats           mean[c] and m2[c] = sum (x - mean)^2 over the R rows.  Each workgroup forms (count, mean, M2) of its
 *                   rows from sums shifted by a value of the data and the partials are combined by the pairwise update in
 *                   fp64 in a fixed order: no cancellation on a map whose mean is large against its spread, no
 *                   floating-point atomics, the same bits on every run.  With invstd given (single-process form) the
 *                   call also does what `finalize` does with count = R.
 *   finalize        invstd = 1 / sqrt(m2 / count + eps); running_mean / running_var (nullable) <- (1 - momentum) * old
 *                   + momentum * (mean | m2 / (count - 1)), as torch.nn.BatchNorm2d updates them.  A multi-process run
 *                   all-reduces (count, mean, m2) between `stats` and this call.
 *   apply           y = relu?((x - mean) * invstd * gamma + beta (+ residual)), one pass; residual nullable.
 *   backward_reduce sum_dy[c] = sum g, sum_dy_xhat[c] = sum g * xhat with g = dy, gated by y > 0 where relu != 0 (y may
 *                   be NULL otherwise): dbeta and dgamma.  A multi-process run all-reduces the two vectors here.
 *   backward_apply  dx = gamma * invstd * (g - sum_dy / count - xhat * sum_dy_xhat / count); dresidual (nullable) = g.
 * workspace: jtsm_batch_norm_workspace_bytes(R, C) for stats and backward_reduce.
 * ------------------------------------------------------------------------- */
size_t jtsm_batch_norm_workspace_bytes(long R, int C);
int jtsm_batch_norm_stats_f32(const float* x, long ld, long R, int C, float* mean, float* m2, float eps, float momentum,
                              float* invstd, float* running_mean, float* running_var, void* workspace, void* stream);
int jtsm_batch_norm_finalize_f32(const float* mean, const float* m2, double count, int C, float eps, float momentum,
                                 float* invstd, float* running_mean, float* running_var, void* stream);
int jtsm_batch_norm_apply_f32(const float* x, long ld, const float* residual, const float* mean, const float* invstd,
                              const float* gamma, const float* beta, float* y, long R, int C, int relu, void* stream);
int jtsm_batch_norm_backward_reduce_f32(const float* x, long ld, const float* dy, const float* y, const float* mean,
                                        const float* invstd, float* sum_dy, float* sum_dy_xhat, void* workspace, long R,
                                        int C, int relu, void* stream);
int jtsm_batch_norm_backward_apply_f32(const float* x, long ld, const float* dy, const float* y, const float* mean,
                                       const float* invstd, const float* gamma, const float* sum_dy,
                                       const float* sum_dy_xhat, double count, float* dx, float* dresidual, long R, int C,
                                       int relu, void* stream);

/* ---------------------------------------------------------------------------
 * DeepLabCE, hard-pixel-mining cross-entropy (projects/DeepLab/deeplab/loss.py:6-40) of the bilinearly xS up-sampled
 * logits (F.interpolate(..., scale_factor=common_stride, mode="bilinear", align_corners=False) in the losses() of
 * projects/DeepLab/deeplab/semantic_seg.py), the full-resolution logits never materialised.  Limits and layout of
 * jtsm_semseg_ce_*: logits (N,Hs,Ws,ld) NHWC, 16-byte aligned, C <= ld <= 64, ld % 4 == 0; target (N,Hs*S,Ws*S) int64.
 * forward: lse and pixel_loss (one float per output pixel; the loss is 0 where the target is ignored and is multiplied
 * by weights[pixel] where weights != NULL); out[0] = mean of the k largest pixel losses = (sum of the losses above the
 * cut t + (k - their number) * t) / k with fp64 sums in a fixed order, out[1] = t.  k is the caller's
 * int(top_k_percent_pixels * pixels), 1 <= k <= pixels, ignored pixels counted; k = pixels is the mean over ALL pixels.
 * The cut is found by a radix select over 8-bit digits of a key that orders every float (-0 = +0, NaN largest: a NaN
 * loss gives a NaN result, as torch.topk), with per-workgroup LDS histograms; the workspace,
 * jtsm_deeplab_ce_workspace_bytes(), does not depend on the sizes.
 * TIES AT THE CUT: among the pixels whose loss equals t, those with the LOWER FLAT INDEX (n, h, w) are chosen first (the
 * reference's topk leaves this open; the same rule as jtsm_retinanet_candidates_f32).
 * coef (one float per output pixel) = chosen * weight / k, 0 for ignored pixels: the backward's per-pixel factor.
 * backward: the deterministic gather of jtsm_semseg_ce_backward_f32 with coef in place of the one upstream scalar;
 * dlogits (N,Hs,Ws,ld) = *upstream (1 if NULL) * d out[0] / d logits, pad lanes zero.
 * ------------------------------------------------------------------------- */
size_t jtsm_deeplab_ce_workspace_bytes(void);
int jtsm_deeplab_ce_forward_f32(const float* logits, int ld, int C, const int64_t* target, const float* weights, long k,
                                float* lse, float* pixel_loss, float* coef, float* out, void* workspace, int N, int Hs,
                                int Ws, int S, long ignore_index, void* stream);
int jtsm_deeplab_ce_backward_f32(const float* logits, int ld, int C, const int64_t* target, const float* lse,
                                 const float* coef, const float* upstream, float* dlogits, int N, int Hs, int Ws, int S,
                                 long ignore_index, void* stream);


/* ---------------------------------------------------------------------------
 * Pseudo-ground-truth mining and proposal labelling (no native reference; PyTorch glue at
 * projects/WSL/wsl/modeling/roi_heads/roi_heads_jtsm.py:1167-1338 (get_pgt_top_k, top_k = 1),
 * roi_heads.py:264-370 (label_and_sample_proposals: pairwise_iou + Matcher([0.5],[0,1]), no
 * sub-sampling), fast_rcnn_oicr.py:684-783 (softmax / apply_deltas of the previous branch)).
 * Proposals of image i are rows [bag_offsets[i], bag_offsets[i+1]); image i has counts[i] <= Gmax
 * present classes, listed in classes[i*Gmax ..].
 * ------------------------------------------------------------------------- */
/* lse[r] = log sum_c exp(logits[r,c]). */
int jtsm_row_lse_f32(const float* logits, int ld, int ncls, int R, float* lse, void* stream);
/* For every (image, present class): the row with the highest score[r,class] (score = scores[r,c], or
 * exp(scores[r,c] - lse[r]) when lse != NULL, i.e. softmax of logits; lowest row wins ties).  Writes the
 * row (relative to the image), its score, the class's image-level probability as weight, and the box:
 * the proposal itself, or (deltas != NULL, (R, ld_deltas) class-major 4-tuples) the proposal decoded with
 * Box2BoxTransform(10,10,5,5).apply_deltas for that class. */
int jtsm_mine_top1_f32(const float* scores, int ld, const float* lse, const float* proposals,
                       const float* deltas, int ld_deltas, const int32_t* bag_offsets,
                       const int32_t* classes, const int32_t* counts, int B, int Gmax,
                       const float* img_probs, int nprob, int32_t* out_idx, float* out_box,
                       float* out_score, float* out_weight, void* stream);
/* Pseudo semantic target (get_pgt_sem_seg, projects/WSL/wsl/modeling/roi_heads/roi_heads_jtsm.py:2025-2070, with
 * the rectangle substitution of SURVEY F8): out (B,H,W) int64 <- 0, then every pseudo box j < counts[b] of image b
 * paints the pixels whose centre lies in its rectangle shrunk by `erode` with classes[b,j] - class_base (1..63), in
 * ascending scores[b,j] order (ties: lower j first); finally, in list order, a class left without a single pixel is
 * painted once more.  boxes (B,G,4), classes / scores (B,G), G <= 64.  workspace: jtsm_paint_sem_seg_workspace_bytes. */
size_t jtsm_paint_sem_seg_workspace_bytes(int B);
int jtsm_paint_sem_seg(const float* boxes, const int32_t* classes, const float* scores, const int32_t* counts,
                       int B, int G, int class_base, int H, int W, float erode, int64_t* out, void* workspace,
                       void* stream);
/* The same target painted from the reference's own masks (roi_heads_jtsm.py:2038-2069: get_pgt_top_k(need_mask=True)
 * -> :1333-1334 object_evidence -> :1928-1994, superpixel branch): target j of image b is proposal row
 * bag_offsets[b] + target_idx[b,j] of oh_labels (R, L) int32, and its mask is the union of the superpixels that row
 * marks: mask_j(y,x) = oh_labels[row_j][superpixels[b,y,x]] != 0 (ids outside [0, L) belong to no mask).  Paint order,
 * values and the second pass for classes left without a pixel as above.  superpixels (B,H,W) int32 at the OUTPUT size. */
int jtsm_paint_sem_seg_evidence(const int32_t* target_idx, const int32_t* bag_offsets, const int32_t* oh_labels, int L,
                                const int32_t* superpixels, const int32_t* classes, const float* scores,
                                const int32_t* counts, int B, int G, int class_base, int H, int W, int64_t* out,
                                void* workspace, void* stream);
/* For every proposal: IoU against its image's pseudo boxes (first maximum wins), label = that box's
 * class if IoU >= iou_thresh else bg_label, plus the matched index / box / weight / (optional) score. */
int jtsm_match_label_f32(const float* proposals, const int32_t* bag_offsets, int B, int R,
                         const float* pgt_box, const int32_t* classes, const int32_t* counts,
                         const float* pgt_weight, const float* pgt_score, int Gmax, float iou_thresh,
                         int bg_label, int32_t* labels, int32_t* matched, float* gt_boxes,
                         float* gt_weights, float* gt_scores, void* stream);

/* ---------------------------------------------------------------------------
 * MIST mining (projects/WSL/wsl/modeling/roi_heads/roi_heads_oicr.py:550-591 get_pgt_mist on get_pgt_top_k :660-811
 * with top_k = top_pro < 1): per image, the top_t[b] rows of every present class by class score, one class-agnostic
 * greedy NMS over all of them, the survivors as a padded pseudo-ground-truth list.  Nothing is read back.
 * Operands as jtsm_mine_top1_f32 takes them (score = scores[r,c], or exp(scores[r,c] - lse[r]) when lse != NULL;
 * deltas != NULL: the class's box decoded as mine_top1 decodes it; deltas == NULL and decode_zero_deltas != 0: the
 * proposal decoded with zero deltas, which is what the reference computes for a branch without regression and differs
 * from the proposal in the last bit; otherwise the proposal row itself).  top_t (B) int32 on the device, host-computed
 * max(int(rows_b * top_pro), 1); t_max >= every top_t[b] (larger entries are cut to t_max, and to the image's rows).
 * Candidate (j, g) — the class slot g's j-th best row, equal scores by lower row — has list index j * counts[b] + g;
 * the NMS visits the list by descending score, equal scores by lower list index, and drops a candidate whose IoU with
 * an earlier survivor is > iou_thresh (the IoU expression of jtsm_batched_nms_f32).  Outputs, P = t_max * G entries
 * per image, survivors in visiting order and zeros behind them: out_boxes (B,P,4), out_classes (B,P), out_scores
 * (B,P), out_weights (B,P) = the scores (:584-586), out_rows (B,P) = the source row within the image, out_num (B).
 * An image with counts[b] == 0 gets out_num[b] = 0.  The list feeds jtsm_match_label_f32 with Gmax = P, counts =
 * out_num.  Deterministic: no atomics.  out_boxes 16-byte, workspace 256-byte aligned.
 * ------------------------------------------------------------------------- */
size_t jtsm_mine_top_p_workspace_bytes(int B, int G, int t_max);
int jtsm_mine_top_p_f32(const float* scores, int ld, const float* lse, const float* proposals,
                        const float* deltas, int ld_deltas, int decode_zero_deltas,
                        const int32_t* bag_offsets, const int32_t* classes, const int32_t* counts,
                        const int32_t* top_t, int B, int G, int t_max, float iou_thresh, float* out_boxes,
                        int32_t* out_classes, float* out_scores, float* out_weights, int32_t* out_rows,
                        int32_t* out_num, void* workspace, void* stream);

/* ---------------------------------------------------------------------------
 * C-MIL (cmil.hip).  Both operators take all images of the step (rows [bag_offsets[b], bag_offsets[b+1]) of every
 * per-row array), compute pairwise_iou's expression where they need an IoU — no R x R matrix — and read nothing back.
 *
 * jtsm_roi_merge_forward_f32 <- ROIMerge_forward_cpu(S, J, C, D, P)
 *   (projects/WSL/wsl/layers/csrc/ROIMerge/ROIMerge_cpu.cpp:33-232): S (R) the rows' summed MIL scores, boxes (R,4) in
 *   place of J, C / D (R,K) with leading dimensions ldc / ldd, lam = getlambda(cur_iter / size_epoch, max_epoch)
 *   (:11-17) evaluated by the caller in place of P.  Per image: rows ranked by S descending (equal S: lower row), the
 *   first min(rows, 200) ranks walked greedily in windows of 40 (a rank joins the seed's clique unless its IoU with a
 *   member is < lam), every other row its own clique in row order.  The cliques of all images are compacted: image
 *   b's clique id is merged row merged_offsets[b] + id.  MC / MD (R,K) contiguous: the clique means, sum over the
 *   members in ascending row order of C[n] / IC, un-contracted; I (R): a row's merged row; IC (R): members of a
 *   merged row; merged_offsets (B+1).  Rows at and behind merged_offsets[B] are dead: MC = MD = 0, IC = 0.
 *   max_bag_rows >= every image's rows (host int).  boxes 16-byte, workspace 256-byte aligned.
 * jtsm_roi_merge_backward_f32 <- ROIMerge_backward_cpu (:234-287): dC[n] = gMC[I[n]] / IC[I[n]], dD likewise; gMC /
 *   gMD (R,K) with leading dimension ld, dC / dD with ld_grad.  Dead rows of gMC / gMD are not read.
 *
 * jtsm_roi_label_f32 <- ROILabel_forward_cpu(S, U, L, CW, P) (.../ROILabel/ROILabel_cpu.cpp:16-194): S (R, ld) class
 *   scores (score = S[r,c], or exp(S[r,c] - lse[r]) when lse != NULL), boxes (R,4) in place of U, classes (B,G) /
 *   counts (B) the present classes ascending in place of L, CW (B, ld_cw) the image probabilities (NULL: the seed's
 *   score is the weight), and fg, bg_hi, bg_lo, num_pos, num_neg, top_k in place of P.  perm (R): for every image a
 *   permutation of 0 .. rows-1 at its rows' positions — the visiting order the reference draws with
 *   srand(time(0)).  Seeds: per present class, top_k times, the best-scoring row no seed holds yet (first maximum);
 *   none once the rows have run out.  Every row takes the seed of largest IoU (first maximum); visited in perm order it
 *   gets the seed's class and weight when IoU >= fg and at most num_pos positives were taken before it, label
 *   num_classes and the weight when bg_lo <= IoU < bg_hi and at most num_neg negatives were taken, otherwise the
 *   seed's class and weight 0 (an image without seeds: num_classes, 0).  fg >= bg_hi is required.  labels (R),
 *   weights (R); seed_rows (B, G * top_k): the seeds' rows within the image in picking order, -1 behind seed_num (B).
 *   At most 256 seeds per image (G * top_k).  boxes 16-byte aligned.
 * Deterministic: no atomics.
 * ------------------------------------------------------------------------- */
size_t jtsm_roi_merge_workspace_bytes(int B, int R);
int jtsm_roi_merge_forward_f32(const float* S, const float* boxes, const float* C, int ldc, const float* D, int ldd,
                               int K, const int32_t* bag_offsets, int B, int R, int max_bag_rows, float lam, float* MC,
                               float* MD, int32_t* I, int32_t* IC, int32_t* merged_offsets, void* workspace,
                               void* stream);
int jtsm_roi_merge_backward_f32(const float* gMC, const float* gMD, int ld, int K, const int32_t* I, const int32_t* IC,
                                int R, float* dC, float* dD, int ld_grad, void* stream);
int jtsm_roi_label_f32(const float* S, int ld, const float* lse, const float* boxes, const int32_t* bag_offsets,
                       const int32_t* classes, const int32_t* counts, int B, int G, const float* CW, int ld_cw,
                       const int32_t* perm, float fg, float bg_hi, float bg_lo, int num_pos, int num_neg, int top_k,
                       int num_classes, int32_t* labels, float* weights, int32_t* seed_rows, int32_t* seed_num,
                       void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Inference / post-processing.  None of these entry points synchronises with the host: counts
 * that depend on the data are written to device memory.
 * ------------------------------------------------------------------------------------------------------------------ */

/* OICROutputLayers.predict_probs_K + predict_boxes_K (projects/WSL/wsl/modeling/roi_heads/fast_rcnn_oicr.py:712-783):
 * probs (R, C1) <- mean over `heads` of softmax(logits[h] (R, C1)); boxes (R, Kb*4) <- Box2BoxTransform(weights)
 * .apply_deltas(mean over heads of deltas[h] (R, Kb*4), proposals (R, 4)) (detectron2/modeling/box_regression.py:78-113).
 * `logits` / `deltas` are HOST arrays of `heads` (<= 8) device pointers; boxes == NULL skips the box part. */
int jtsm_oicr_predict_f32(const float* const* logits, const float* const* deltas, int heads, int R, int C1, int Kb,
                          const float* proposals, const float* weights /* host, 4 */, float scale_clamp, float* probs,
                          float* boxes, void* stream);

/* batched_nms (detectron2/layers/nms.py:10-31 -> torchvision.ops.boxes.batched_nms / nms, pinned 0.8.1 by
 * docker/Dockerfile:25): greedy NMS within each class.  boxes (n,4) xyxy, scores (n), idxs (n) int64 in
 * [0, num_classes) (anything else drops the element), max_per_class >= the largest class population.
 * coordinate_trick: 1 = torchvision's `boxes + idxs * (boxes.max() + 1)` fp32 offsets (the n < 40000 branch),
 * 0 = plain per-class NMS (the n >= 40000 branch), 2 = choose by the number of valid elements as nms.py does.
 * keep (n) int64 <- element indices, survivors first in descending score order (equal scores: lower index first),
 * *num_keep (device) <- number of survivors; *overflow (device, optional) <- 1 if a class exceeded max_per_class
 * (the result is then invalid).  IoU test: inter / (area_a + area_b - inter) > iou_threshold, as nms_cuda.cu. */
size_t jtsm_batched_nms_workspace_bytes(int n, int num_classes, int max_per_class);
int jtsm_batched_nms_f32(const float* boxes, const float* scores, const int64_t* idxs, int n, int num_classes,
                         int max_per_class, float iou_threshold, int coordinate_trick, int64_t* keep,
                         int32_t* num_keep, int32_t* overflow, void* workspace, size_t workspace_bytes, void* stream);

/* Rotated boxes (cx, cy, w, h, angle in degrees): detectron2/layers/rotated_boxes.py:6-21 pairwise_iou_rotated ->
 * csrc/box_iou_rotated/box_iou_rotated_cuda.cu, and detectron2/layers/nms.py:35-139 nms_rotated / batched_nms_rotated
 * -> csrc/nms_rotated/nms_rotated_cuda.cu.  The IoU of a pair is the device branch of box_iou_rotated_utils.h, every
 * operation rounded on its own (no fused multiply-add), in that header's types.
 *
 * jtsm_box_iou_rotated_f32: ious (N,M) <- IoU of boxes1 (N,5) and boxes2 (M,5).  N == 0 or M == 0: nothing to do.
 *
 * jtsm_batched_nms_rotated_f32: greedy NMS within each class.  boxes (n,5), scores (n), idxs (n) int64 in
 * [0, num_classes) (anything else drops the element) or NULL: one class (num_classes must be 1; that is nms_rotated).
 * Classes are segments of the sorted list and the boxes are NOT offset: the reference's `boxes + idxs * (max - min +
 * 1)` on the fp32 centres is a way to the same separation that perturbs the centres' low bits.  max_per_class, keep
 * (survivors first, descending score, equal scores: lower index first), *num_keep (device), *overflow (device,
 * optional) and "nothing is read back" as jtsm_batched_nms_f32.  IoU test: iou > iou_threshold, as
 * nms_rotated_cuda.cu (the reference's CPU kernel tests >=). */
int jtsm_box_iou_rotated_f32(const float* boxes1, const float* boxes2, int N, int M, float* ious, void* stream);
size_t jtsm_batched_nms_rotated_workspace_bytes(int n, int num_classes, int max_per_class);
int jtsm_batched_nms_rotated_f32(const float* boxes, const float* scores, const int64_t* idxs, int n, int num_classes,
                                 int max_per_class, float iou_threshold, int64_t* keep, int32_t* num_keep,
                                 int32_t* overflow, void* workspace, size_t workspace_bytes, void* stream);

/* fast_rcnn_inference_single_image (projects/WSL/wsl/modeling/roi_heads/fast_rcnn_oicr.py:100-163) in one call:
 * rows with a non-finite box or score are dropped, boxes (R, Kb*4), Kb in {1, K}, are clipped to (img_h, img_w),
 * every (row, class < K) with scores (R, K+1) > score_thresh becomes a candidate, batched_nms (above, trick mode 2),
 * top `topk` (< 0: all).  Outputs have `cap` slots (unused slots: zeros / -1): boxes (cap,4), scores, classes,
 * rows (the proposal row of each detection) and *out_count (device). */
size_t jtsm_fast_rcnn_inference_workspace_bytes(int R, int K);
int jtsm_fast_rcnn_inference_f32(const float* boxes, const float* scores, int R, int K, int Kb, float img_h,
                                 float img_w, float score_thresh, float nms_thresh, int topk, int cap,
                                 float* out_boxes, float* out_scores, int64_t* out_classes, int64_t* out_rows,
                                 int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream);

/* mask_rcnn_inference (projects/WSL/wsl/modeling/roi_heads/mask_head.py:106-147) on the head average of
 * roi_heads_jtsm.py:949-961: out (N, M, M) <- sigmoid((sum_h logits[h][n, c_n]) / heads), c_n = classes[n] (0 when
 * C == 1).  `logits`: HOST array of device pointers to (N, C, M, M). */
int jtsm_mask_probs_f32(const float* const* logits, int heads, const int64_t* classes, int N, int C, int M,
                        float* out, void* stream);

/* paste_masks_in_image (detectron2/layers/mask_ops.py:74-145; GPU branch of _do_paste_mask :17-71): out (N, img_h,
 * img_w) <- grid_sample(masks (N, M, M), bilinear, zeros, align_corners=False) over the whole image, then
 * `>= threshold` as 0/1 (threshold >= 0) or `* 255` truncated to uint8 (threshold < 0). */
int jtsm_paste_masks_f32(const float* masks, const float* boxes, int N, int M, int img_h, int img_w, float threshold,
                         uint8_t* out, void* stream);

/* F.interpolate(x[..., :crop_h, :crop_w], mode="bilinear", align_corners=False) into planar y (N, C, out_h, out_w);
 * scale_h / scale_w are the source-index scales (1 / scale_factor, or crop / out): SemSegFPNHead's x common_stride
 * upsampling (detectron2/modeling/meta_arch/semantic_seg.py:172-176) and sem_seg_postprocess
 * (detectron2/modeling/postprocessing.py:75-100). */
int jtsm_resize_bilinear_f32(const float* x, int layout, int N, int C, int H, int W, int crop_h, int crop_w,
                             int out_h, int out_w, float scale_h, float scale_w, float* y, void* stream);
/* F.interpolate(x, size=(out_h, out_w), mode="nearest") of a planar (C, H, W) map, optionally reading the source
 * columns mirrored: the resize + un-flip of GeneralizedRCNNWithTTAAVG._reduce_pred_sem_seg
 * (projects/WSL/wsl/modeling/test_time_augmentation_avg.py:428-442; ResizeTransform.apply_segmentation on float
 * arrays, detectron2/data/transforms/transform.py:116-141). */
int jtsm_resize_nearest_f32(const float* x, int C, int H, int W, int out_h, int out_w, int flip_source, float* y,
                            void* stream);
/* out (HW) int64 <- argmax over c of planar x (C, HW); first maximum wins (sem_seg_r.argmax(dim=0), mcnn.py:352). */
int jtsm_argmax_channels_f32(const float* x, int C, long HW, int64_t* out, void* stream);

/* combine_semantic_and_instance_outputs (detectron2/modeling/meta_arch/panoptic_fpn.py:133-218).  masks (N, H, W)
 * uint8, order (N) int32 = instance indices by descending score, scores / classes (N), sem (H, W) int64 in [0, S),
 * S <= 256.  panoptic (H, W) int32 <- segment ids; seg_table (N + S, 5) int32 rows {id, isthing, category_id,
 * instance_id or -1, area (stuff: unpainted area; things: newly painted pixels)}, seg_score (N + S),
 * *num_segments (device).  max_visits: number of leading instances (in `order`) to walk — pass the count of scores
 * >= the confidence threshold when it is known, or -1 for all N (the walk itself stops at the threshold too). */
size_t jtsm_panoptic_combine_workspace_bytes(int N, int S);
int jtsm_panoptic_combine(const uint8_t* masks, const int32_t* order, const float* scores, const int64_t* classes,
                          int N, int H, int W, const int64_t* sem, int S, double overlap_threshold,
                          int stuff_area_limit, float instances_confidence_threshold, int32_t* panoptic,
                          int32_t* seg_table, float* seg_score, int32_t* num_segments, int max_visits,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Pascal VOC detection AP at IoU 0.50:0.05:0.95 and CorLoc: PascalVOCDetectionEvaluator.process / evaluate with
 * voc_eval, voc_ap and voc_eval_corloc (detectron2/evaluation/pascal_voc_evaluation.py:55-69, 210-355, 358-452) for all
 * classes and thresholds in one call that reads nothing back.  Semantics: scores and boxes are first
 * quantised to what the reference prints and parses again (thousandths; tenths, xmin / ymin after an fp32 + 1); fp64
 * from there on; detections of a class are ranked by descending quantised score, equal scores in input order.
 * Detections: det_boxes (D,4) xyxy as the model gives them (0-based), det_scores (D), det_classes (D) in [0, C),
 * det_images (D) in [0, N).  Ground truth: gt_boxes (G,4) int32 as in the XML (1-based), gt_difficult (G) uint8, sorted
 * by (class, image); gt_offsets (C*N+1) the CSR over (class, image), class-major.  C < 65536, N <= 2^24 (the bits the
 * sort keys give them), else JTSM_EINVAL.
 * Outputs: ap (10,C) and corloc (10,C) double, fractions (not x100), row t = threshold (50 + 5t)/100; ap is the 11-point
 * form when use_07_metric != 0, else the area form (NaN for a class with detections and no non-difficult ground truth,
 * as the reference; the 11-point form gives 0).  corloc is 0 for a class without detections and NaN for a class with
 * detections and no image holding a non-difficult box (the reference divides by zero).  counts (C,2) int32 = {npos,
 * npos_im}.  stats (4) double = {smallest score, largest score, number of detections whose class or image index is out
 * of range (they are left out of everything), 0}.  Optional (NULL to skip), each (D) in INPUT order: tp_bits / fp_bits
 * uint16 with bit t = the detection is a true / false positive at threshold t; order int32 = the detection's position
 * in its class's ranking (-1 for an out-of-range detection).
 * det_boxes and gt_boxes 16-byte aligned, workspace 256-byte aligned.  Integer atomics only: deterministic.
 * ------------------------------------------------------------------------------------------------------------------ */
size_t jtsm_voc_eval_workspace_bytes(int D, int G, int C);
int jtsm_voc_eval(const float* det_boxes, const float* det_scores, const int32_t* det_classes,
                  const int32_t* det_images, int D, const int32_t* gt_boxes, const uint8_t* gt_difficult,
                  const int32_t* gt_offsets, int G, int N, int C, int use_07_metric, double* ap, double* corloc,
                  int32_t* counts, double* stats, uint16_t* tp_bits, uint16_t* fp_bits, int32_t* order,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Panoptic quality and the semantic confusion matrix on the device: what COCOPanopticEvaluator.process / evaluate do
 * through PNG files and panopticapi.pq_compute (detectron2/evaluation/panoptic_evaluation.py:66-144) and what
 * SemSegEvaluator.process does with one np.bincount per image (detectron2/evaluation/sem_seg_evaluation.py:82-93), on
 * the maps where inference left them.  Semantics: DESIGN.md §4f (pq_compute_single_core of panopticapi).
 *
 * jtsm_pq_accumulate — ONE image per call, added into running per-category totals that stay on the device.
 *   pred (pixels) int32 panoptic ids as jtsm_panoptic_combine writes them, 0 = VOID; pred_table (P,5) int32 rows {id,
 *   isthing, category_id, instance_id, area} of which the first min(*num_pred, P) count (num_pred on the device; column
 *   0 is looked up per pixel — ids need not be dense; column 4 is ignored, areas are counted); thing_cat (num_things) /
 *   stuff_cat (num_stuff) int32: contiguous id -> evaluation category in [0, C), or -1.  gt (pixels) int32: 0 = VOID,
 *   r + 1 = row r of gt_table (G,2) int32 {category in [0, C), iscrowd}.
 *   Totals, added to (zero them before the first image): tp, fp, fn (C) int64; iou_sum (C) double, added sequentially
 *   in gt-row order — bit-reproducible, equal to a sequential fp64 loop over (image, gt row); stats (4) int64 =
 *   {pixels whose non-zero value names no row (either map; counted as VOID), rows of pred_table without a pixel, rows
 *   (either table) whose category is -1 or out of range (left out of matching, fp and fn), images accumulated}.
 *   The (G+1) x (P+1) pair histogram is built in LDS while it has at most jtsm_pq_lds_cells() counters, with global
 *   atomics above (force_global != 0: always); both give the same integers.  (G+1)(P+1) <= 2^28, else JTSM_EINVAL.
 *   workspace: jtsm_pq_accumulate_workspace_bytes(G, P, C), 256-byte aligned.
 *
 * jtsm_confusion_accumulate — conf[(C+1) * pred + gt'] += 1 per pixel, conf (C+1)^2 int64 with C = num_classes; pred
 *   (pixels) int64 as jtsm_argmax_channels_f32 writes it; gt (pixels) uint8 or int32 (gt_elem_bytes 1 or 4); gt' = C
 *   where gt == ignore_label.  A pixel whose pred is outside [0, C) or whose gt' is outside [0, C] is counted in
 *   *stats (int64) and left out (np.bincount would raise or grow).  LDS histogram while (C+1)^2 <=
 *   jtsm_confusion_lds_cells(), global atomics above (force_global != 0: always).
 * Integer atomics only; maps are read with 16-byte loads when their addresses allow.
 * ------------------------------------------------------------------------------------------------------------------ */
int jtsm_pq_lds_cells(void);
int jtsm_confusion_lds_cells(void);
size_t jtsm_pq_accumulate_workspace_bytes(int G, int P, int C);
int jtsm_pq_accumulate(const int32_t* pred, const int32_t* pred_table, const int32_t* num_pred, int P,
                       const int32_t* thing_cat, int num_things, const int32_t* stuff_cat, int num_stuff,
                       const int32_t* gt, const int32_t* gt_table, int G, long pixels, int C, int64_t* tp, int64_t* fp,
                       int64_t* fn, double* iou_sum, int64_t* stats, int force_global, void* workspace,
                       size_t workspace_bytes, void* stream);
int jtsm_confusion_accumulate(const int64_t* pred, const void* gt, int gt_elem_bytes, long pixels, int num_classes,
                              int ignore_label, int64_t* conf, int64_t* stats, int force_global, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * COCO box / mask AP on the device: COCOEvaluator's bbox and segm tasks (detectron2/evaluation/coco_evaluation.py) as
 * COCOeval_opt computes them (evaluation/fast_eval_api.py; layers/csrc/cocoeval/cocoeval.cpp: EvaluateImages,
 * Accumulate) with pycocotools' default parameters, and the keypoints task (OKS).  Semantics: DESIGN.md §4g.  T = 10
 * IoU thresholds and A = 4 area ranges are fixed; bit a * 10 + t of a record word belongs to (area range a, threshold
 * t).
 *
 * jtsm_coco_image — ONE image and ONE task per call: ranks, IoUs and matches of the image's detections, one 32-byte
 *   record each, and the image's non-ignored ground truth added into npos.
 *   det_boxes (n,4) float32 XYXY, det_scores (n), det_classes (n) int32 in [0, K) (another value: counted in stats[0],
 *   the detection is left out); det_masks (n, H, W) uint8 / bool, non-zero = set, or NULL.  Ground truth of the image
 *   sorted by category, annotation order inside: gt_boxes (G,4) double XYWH, gt_area (G) double (the annotation's area
 *   field), gt_crowd (G) uint8 (ignore := iscrowd), gt_cat_start (K+1) int32 CSR over the categories, gt_masks (G,
 *   ceil(H W / 64)) 64-bit words — pixel p of the flat map is bit p % 64 of word p / 64, tail zero — or NULL.  The
 *   task is segm when det_masks or gt_masks is given (then both where n > 0 / G > 0), else bbox.
 *   iou_thrs (10) and area_rng (4,2) double ON THE DEVICE, used as passed.  max_det: detections kept per (image,
 *   category), <= 128.
 *   records (n, 4) int64 <- {int32 category (K: left out — a bad class or rank >= max_det), int32 image_index, int32
 *   rank, float32 score, uint64 matched bits, uint64 ignore bits}, detection row order.  npos (K, 4) int64 and stats
 *   (2) int64 are ADDED to (zero them before the first image).
 *   Optional (NULL to skip): ious_debug (n, G) double <- the IoU of every same-category pair of a kept detection, -1
 *   elsewhere; rank_debug (n) int32 <- rank or -1.
 *   n <= 65535, G <= 4096 (one matched bit per 64 ground-truth rows in a lane's word), n G <= 2^28, else JTSM_EINVAL.
 *   workspace: jtsm_coco_image_workspace_bytes(n, G, K, H, W, max_det) (H = W = 0 for bbox), 256-byte aligned.
 *
 * jtsm_coco_image_keypoints — the same for the keypoints task: the similarity is pycocotools' computeOks (OKS) in
 *   place of the IoU.  det_keypoints (n, P, 3) float32 (x, y, score) as the model leaves them: x and y get
 *   instances_to_coco_json's `- 0.5` in fp32 where they are read, the array is not written.  gt_keypoints (G, P, 3)
 *   double (x, y, v) as the COCO JSON holds them, rows as gt_boxes; sigmas (P) double on the device.  gt_ignore (G)
 *   uint8 is the annotation's ignore flag (iscrowd or num_keypoints == 0: never counted, a match to it is ignored),
 *   gt_crowd (G) uint8 only says which objects may be matched more than once.  The detection's area is w * h of its
 *   box, as for bbox.  area_rng keeps four rows: the keypoints task's three plus a spare that repeats one of them.
 *   1 <= P <= 64 and jtsm_coco_image's limits, else JTSM_EINVAL.  ious_debug <- the OKS.
 *   workspace: jtsm_coco_image_keypoints_workspace_bytes(n, G, K, P, max_det), 256-byte aligned.
 *
 * jtsm_coco_accumulate — the precision / scores (10, R, K, 4, M) and recall (10, K, 4, M) double tables, -1 where a
 *   (category, area range) has no non-ignored ground truth, from the concatenated records (D, 4) of all images, in any
 *   order: image_index in [0, N) must rise with the image id.  rec_thrs (R <= 1024) double and max_dets (M <= 8) int32
 *   on the device.  bits(K) + bits(N-1) <= 25 (the sort key beside 32 score and 7 rank bits), else JTSM_EINVAL.
 * Integer atomics only: deterministic.  Nothing is allocated or synchronised.
 * ------------------------------------------------------------------------------------------------------------------ */
size_t jtsm_coco_image_workspace_bytes(int n, int G, int K, int H, int W, int max_det);
int jtsm_coco_image(const float* det_boxes, const float* det_scores, const int32_t* det_classes,
                    const uint8_t* det_masks, int n, int H, int W, const double* gt_boxes, const double* gt_area,
                    const uint8_t* gt_crowd, const int32_t* gt_cat_start, const uint64_t* gt_masks, int G, int K,
                    int image_index, int max_det, const double* iou_thrs, const double* area_rng, int64_t* records,
                    int64_t* npos, int64_t* stats, double* ious_debug, int32_t* rank_debug, void* workspace,
                    size_t workspace_bytes, void* stream);
size_t jtsm_coco_image_keypoints_workspace_bytes(int n, int G, int K, int P, int max_det);
int jtsm_coco_image_keypoints(const float* det_boxes, const float* det_scores, const int32_t* det_classes,
                              const float* det_keypoints, int n, int P, const double* gt_boxes, const double* gt_area,
                              const uint8_t* gt_crowd, const uint8_t* gt_ignore, const double* gt_keypoints,
                              const int32_t* gt_cat_start, int G, int K, const double* sigmas, int image_index,
                              int max_det, const double* iou_thrs, const double* area_rng, int64_t* records,
                              int64_t* npos, int64_t* stats, double* ious_debug, int32_t* rank_debug, void* workspace,
                              size_t workspace_bytes, void* stream);
size_t jtsm_coco_accumulate_workspace_bytes(int D, int K);
int jtsm_coco_accumulate(const int64_t* records, int D, int K, int N, const int64_t* npos, const double* rec_thrs,
                         int R, const int32_t* max_dets, int M, double* precision, double* scores, double* recall,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Deformable convolution v1 / v2: the sampling kernels of detectron2/layers/csrc/deformable/deform_conv_cuda_kernel.cu
 * (deformable_im2col / modulated_deformable_im2col, *_col2im_coord, *_col2im) around this library's own contraction.
 * Semantics and the reasons for the gather form: DESIGN.md §4j.  All tensors float32 and channels-last:
 *   x (N, H, W, C); offset (N, Ho, Wo, G * 2 * K) and mask (N, Ho, Wo, G * K) — logical (N, channels, Ho, Wo) with the
 *   reference's channel meaning: inside deformable group g, channel 2 k is dy and 2 k + 1 is dx of tap k = i * kw + j;
 *   mask == NULL: v1 (no modulation).  K = kh * kw, G = deformable_groups, C / G a multiple of 4; stride, pad and
 *   dil are square; Ho = (H + 2 pad - dil (kh - 1) - 1) / stride + 1, Wo likewise.
 *   cols / dcols (N * Ho * Wo, K, C): tap-major, channel-minor rows — a channels-last (O, C, kh, kw) weight viewed as
 *   (O, K * C) contracts them with no repacking.
 *
 * jtsm_deform_columns_f32 — cols <- mask * bilinear(x, p), p = ((float)(oy stride - pad + i dil) + dy, ... + dx); a
 *   sample counts only inside (-1, H) x (-1, W), a corner only inside the map; w1 v1 + w2 v2 + w3 v3 + w4 v4 summed
 *   left to right, the mask multiplied last (bit-defined: the file is built without floating-point contraction).
 * jtsm_deform_offset_mask_grad_f32 — d_offset (offset's layout) <- sum over the group's channels of dcols * mask *
 *   coordinate weight; d_mask (mask's layout; NULL with mask == NULL) <- sum of dcols * bilinear(x).  A fixed-shape
 *   reduction per (pixel, tap, group): no atomics, every element written.
 * jtsm_deform_input_grad_f32 — dx (N, H, W, C) <- the transposed sampling of dcols, as a deterministic gather: one
 *   64-bit key per (sample, corner) with the destination in the high bits, a stable radix sort, one workgroup per
 *   destination walking its list in order.  EVERY element of dx is written (destinations nothing reaches get zero): the
 *   caller does not clear it.  workspace: jtsm_deform_input_grad_workspace_bytes(...), 256-byte aligned.  4 N Ho Wo K G
 *   and N H W G must stay below 2^31, else JTSM_EINVAL (the caller loops over groups of images).
 * Nothing is allocated or synchronised.
 * ------------------------------------------------------------------------------------------------------------------ */
int jtsm_deform_columns_f32(const float* x, const float* offset, const float* mask, float* cols, int N, int H, int W,
                            int C, int G, int kh, int kw, int stride, int pad, int dil, void* stream);
int jtsm_deform_offset_mask_grad_f32(const float* dcols, const float* x, const float* offset, const float* mask,
                                     float* d_offset, float* d_mask, int N, int H, int W, int C, int G, int kh, int kw,
                                     int stride, int pad, int dil, void* stream);
size_t jtsm_deform_input_grad_workspace_bytes(int N, int H, int W, int G, int kh, int kw, int stride, int pad, int dil);
int jtsm_deform_input_grad_f32(const float* dcols, const float* offset, const float* mask, float* dx, int N, int H,
                               int W, int C, int G, int kh, int kw, int stride, int pad, int dil, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Keypoint R-CNN.  Logits / heatmaps are float32, plain contiguous (R, K, S, S): one (roi, keypoint)
 * map is one row of S * S floats, S <= 64.  rois (R, 4) are x1, y1, x2, y2.  Built without floating-point contraction.
 *
 * jtsm_keypoint_targets_f32 — `_keypoints_to_heatmap`, detectron2/structures/keypoints.py:84-140, in its fp32
 *   arithmetic: scale = (1 / (x2 - x1)) * S, as torch evaluates the reference's `S / (x2 - x1)`; cell = floor((x - x1) * scale); x == x2 -> S - 1; valid = inside and v > 0;
 *   targets (N, K) int32 = (cy * S + cx) * valid; valid (N, K) uint8.  keypoints (N, K, 3) = x, y, v.
 * jtsm_keypoint_loss_forward_f32 / _backward_f32 — `keypoint_rcnn_loss`, detectron2/modeling/roi_heads/
 *   keypoint_head.py:40-96: loss <- sum over valid rows of lse(row) - row[target], divided by `normalizer`, or by the
 *   number of valid rows when normalizer <= 0 (the reference's None); no valid row: 0.  One workgroup per row, the
 *   row in registers, a fixed-order sum over the rows: two runs give the same bits.  workspace:
 *   jtsm_keypoint_loss_workspace_bytes(N, K), 256-byte aligned, carried from the forward to the backward (each row's
 *   lse and the divisor).  Backward: grad_logits <- (exp(x - lse) - onehot) * *grad_loss / divisor on valid rows, 0
 *   on the others; EVERY element is written.  grad_loss is a device scalar.
 * jtsm_keypoint_decode_f32 — `heatmaps_to_keypoints`, detectron2/structures/keypoints.py:143-217: out (R, K, 4) =
 *   x, y, logit, score.  One workgroup per map, the map in LDS; the bicubic value (A = -0.75, align_corners = False,
 *   taps clamped to the border, horizontal sums first) of every pixel of the ceil(w) x ceil(h) up-sampling is
 *   computed on the fly under a running arg-max whose ties go to the lowest flat index; score = 1 / sum exp(map - max)
 *   over the S x S map.  A box side beyond 16384 px is walked up to 16384.  The maps are not modified.
 * jtsm_keypoint_upsample_forward_f32 / _backward_f32 — the tail of `KRCNNConvDeconvUpsampleHead.layers`,
 *   keypoint_head.py:247-272: z (R, H, W, Cp) channels-last is the 3x3 convolution form of ConvTranspose2d(C, K, 4,
 *   stride 2, padding 1), channel (py * 2 + px) * K + k = output pixel (2 i + py, 2 j + px) of keypoint k, Cp >= 4 K
 *   (padding channels ignored); logits (R, K, 4 H, 4 W) <- F.interpolate(scale_factor=2, "bilinear",
 *   align_corners=False) of the shuffled map, one pass.  Backward: grad_z (R, H, W, Cp) <- the exact adjoint as a
 *   gather per element, zeros in the padding channels; no atomics.
 * Nothing is allocated or synchronised; R = 0 / N = 0 launch nothing (the loss forward still writes loss = 0).
 * ------------------------------------------------------------------------------------------------------------------ */
int jtsm_keypoint_targets_f32(const float* keypoints, const float* rois, int N, int K, int S, int32_t* targets,
                              uint8_t* valid, void* stream);
size_t jtsm_keypoint_loss_workspace_bytes(int N, int K);
int jtsm_keypoint_loss_forward_f32(const float* logits, const int32_t* targets, const uint8_t* valid, int N, int K,
                                   int S, float normalizer, float* loss, void* workspace, void* stream);
int jtsm_keypoint_loss_backward_f32(const float* logits, const int32_t* targets, const uint8_t* valid, int N, int K,
                                    int S, const float* grad_loss, const void* workspace, float* grad_logits,
                                    void* stream);
int jtsm_keypoint_decode_f32(const float* maps, const float* rois, int R, int K, int S, float* out, void* stream);
int jtsm_keypoint_upsample_forward_f32(const float* z, int R, int K, int H, int W, int Cp, float* logits,
                                       void* stream);
int jtsm_keypoint_upsample_backward_f32(const float* grad_logits, int R, int K, int H, int W, int Cp, float* grad_z,
                                        void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * RetinaNet.  Built without floating-point contraction.  Nothing is allocated and nothing
 * synchronises with the host; data-dependent counts stay on the device.
 *
 * The level table.  The head's outputs are read where the convolutions wrote them: `logits` / `deltas` are HOST arrays
 * of L (<= 8) device pointers, one per level, and `geom` is a HOST array of L rows of six int64:
 *   cells (= H * W), anchor_offset (first row of the level in R), logits image stride, logits cell stride,
 *   deltas image stride, deltas cell stride                                                    (strides in floats).
 * A cell holds A rows of K logits (4 deltas) back to back; the floats of a cell beyond A * K (4 A) are padding, as
 * conv2d_padded leaves behind bbox_pred's 36 channels.  Row cell * A + a of level l is anchor anchor_offset[l] + it:
 * `permute_to_N_HWA_K` (retinanet.py:27-36) as a view.  A plain (N, HWA, K) tensor with a row stride is A = 1.
 * 16-byte accesses are used where K % 4 == 0 and every pointer, cell stride and image stride is a multiple of four
 * floats; one float at a time otherwise.
 *
 * jtsm_retinanet_label_anchors_f32 — `RetinaNet.label_anchors` (retinanet.py:353-397) with `Matcher.__call__` and
 *   `set_low_quality_matches_` (modeling/matcher.py:61-126) for the whole batch.  anchors (R, 4); gt_boxes (G, 4) and
 *   gt_classes (G) int64 concatenated over images, gt_offsets (N + 1) int32 ON THE DEVICE; `thresholds`
 *   (num_thresholds, ascending, without the matcher's -inf / +inf ends) and `interval_labels` (num_thresholds + 1, each
 *   -1 / 0 / 1) are HOST arrays.  labels (N, R) int32 <- -1 ignore, 0 .. K - 1, K background; matched (N, R) int32 <-
 *   the gt row within the image with the largest IoU, the LOWEST among equals (0 without gt); *num_pos (device) <-
 *   anchors with 0 <= label < K over the batch.  IoU = pairwise_iou (box_iou, box_math.h).  An anchor whose IoU with
 *   some gt equals that gt's maximum over all anchors is positive whatever its interval, with its own arg-max as
 *   `matched` — so a gt that overlaps no anchor (maximum 0, e.g. zero area) turns every anchor that overlaps none
 *   positive, as the reference does.  The per-gt maximum is an integer atomic max over the bits of non-negative
 *   floats; no G x R matrix is stored (the IoUs are formed twice); gt boxes go through LDS 256 at a time.
 *   workspace: jtsm_retinanet_label_workspace_bytes(G).
 *
 * jtsm_retinanet_loss_forward_f32 / _backward_f32 — `RetinaNet.losses` (retinanet.py:287-351):
 *   loss_cls <- sum over anchors with label >= 0 and all K classes of fvcore's sigmoid_focal_loss (target 1 at the
 *   label's class; alpha < 0: no alpha term; gamma 0 and 2 without pow), loss_box_reg <- sum over positive anchors of
 *   smooth_l1(deltas, Box2BoxTransform(weights).get_deltas(anchor, gt_boxes[gt_offsets[n] + matched]), beta)
 *   (beta < 1e-5: L1), both divided by the fp32 value of *normalizer (one double on the device).  training != 0 first
 *   updates *normalizer <- momentum * *normalizer + (1 - momentum) * max(*num_pos, 1), in fp64.  Sums: fp64
 *   per-workgroup partials and one fixed-order final pass — the same inputs give the same bits.  workspace:
 *   jtsm_retinanet_loss_workspace_bytes(), carried to the backward (it keeps the divisor the forward used).
 *   Backward: grad_logits / grad_deltas are HOST arrays of L device pointers to maps laid out as `grad_geom` says
 *   (the inputs' cells and cell strides; image strides that hold whole cells); EVERY float of every cell is written — the closed-form derivative times
 *   *grad_cls (*grad_box_reg, device scalars) / the saved divisor, zeros for ignored anchors, for the deltas of
 *   non-positive anchors and in the padding.  weights: HOST array of 4.
 *
 * jtsm_retinanet_candidates_f32 — the per-level part of `inference_single_image` (retinanet.py:453-481) for every
 *   image and level: keep sigmoid(x) > score_thresh (a NaN never passes), the `topk` best of each (image, level) by
 *   score, EQUAL fp32 SCORES BY LOWER FLAT INDEX anchor * K + class FIRST (the reference's sort leaves that order
 *   open), decoded by apply_deltas(weights, scale_clamp) in decode_box's order.  Outputs have N * L * topk slots,
 *   slot (n * L + l) * topk + place: boxes (.., 4), scores, classes int64 (-1 in unused slots, which
 *   jtsm_batched_nms_f32 drops), rows int32 (optional: the anchor's row within its level, -1 unused), counts (N * L) int32.  The cut is found by a radix select over 16-bit digits of the
 *   key (score bits, inverted flat index): the workspace, jtsm_retinanet_candidates_workspace_bytes(N, L, topk), is
 *   one 65536-bin histogram and topk keys per (image, level) whatever passes the threshold.
 * ------------------------------------------------------------------------------------------------------------------ */
size_t jtsm_retinanet_label_workspace_bytes(int total_gt);
int jtsm_retinanet_label_anchors_f32(const float* anchors, int R, const float* gt_boxes, const int32_t* gt_offsets,
                                     const int64_t* gt_classes, int N, int total_gt, const float* thresholds,
                                     const int32_t* interval_labels, int num_thresholds, int num_classes,
                                     int32_t* labels, int32_t* matched, int32_t* num_pos, void* workspace,
                                     void* stream);
size_t jtsm_retinanet_loss_workspace_bytes(void);
int jtsm_retinanet_loss_forward_f32(const float* const* logits, const float* const* deltas, const int64_t* geom,
                                    int L, int N, int A, int K, int R, const int32_t* labels, const int32_t* matched,
                                    const float* anchors, const float* gt_boxes, const int32_t* gt_offsets,
                                    float alpha, float gamma, float beta, const float* weights,
                                    const int32_t* num_pos, double* normalizer, double momentum, int training,
                                    float* loss_cls, float* loss_box_reg, void* workspace, void* stream);
int jtsm_retinanet_loss_backward_f32(const float* const* logits, const float* const* deltas, const int64_t* geom,
                                     int L, int N, int A, int K, int R, const int32_t* labels, const int32_t* matched,
                                     const float* anchors, const float* gt_boxes, const int32_t* gt_offsets,
                                     float alpha, float gamma, float beta, const float* weights,
                                     const float* grad_cls, const float* grad_box_reg, const void* workspace,
                                     float* const* grad_logits, float* const* grad_deltas, const int64_t* grad_geom,
                                     void* stream);
size_t jtsm_retinanet_candidates_workspace_bytes(int N, int L, int topk);
int jtsm_retinanet_candidates_f32(const float* const* logits, const float* const* deltas, const int64_t* geom, int L,
                                  int N, int A, int K, int R, const float* anchors, const float* weights,
                                  float scale_clamp, float score_thresh, int topk, float* boxes, float* scores,
                                  int64_t* classes, int32_t* rows, int32_t* counts, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * PointRend.  Built without floating-point contraction.  Nothing is allocated and nothing synchronises
 * with the host.  Every bilinear read is ATen's grid_sample with align_corners = False and zero padding, in fp32 in
 * its order: source = ((2 p - 1 + 1) * size - 1) / 2, weights (x1 - x)(y1 - y) ..., taps added nw, ne, sw, se.
 *
 * The source table.  `maps` is a HOST array of L (<= 8) device pointers, `scales` a HOST array of L floats and `geom` a
 * HOST array of L rows of nine int64:  H, W, C, first output column, kind, and the strides in floats of the map's
 * image (or roi), channel, row and column.  kind 0 is a feature map shared by the rois of an image: it is indexed by
 * roi_image[r] (0 .. num_images - 1; any other value reads zeros) and read at the image-space point divided by (W, H) / scale.  kind 1 is a map per roi (the coarse
 * logits): it is indexed by r and read at the box-normalised point; its scale is ignored.
 *
 * The points.  grid_side == 0: `points` (R, P, 2), box-normalised.  grid_side > 0: P == grid_side^2 and point q of
 * every roi is cell q of `generate_regular_grid_point_coords` (point_features.py:54-69), row-major or, with
 * space_to_depth != 0 (even sides), in the order ((by * side/2 + bx) * 2 + dy) * 2 + dx of cell (2 by + dy, 2 bx + dx).
 *
 * jtsm_point_gather_forward_f32 — `point_sample_fine_grained_features` + `point_sample` (point_features.py:28-51,
 *   155-225) for all rois, images and sources in one launch: row r * P + q of `rows` (row_stride floats apart) gets
 *   the C channels of source l in columns col_l .. col_l + C_l; other columns are not touched.  coords_wrt_image
 *   (R, P, 2, optional) <- `get_point_coords_wrt_image`.
 * jtsm_point_gather_backward_roi_f32 — the gradient of a kind-1 source: one workgroup per roi, every cell of the
 *   roi's (C, H, W) map walks the roi's points in order.  Every cell is written, at the given strides.
 * jtsm_point_gather_backward_map_f32 — the gradient of a kind-0 source into a dense channels-last (N, H, W, C) map:
 *   tap records keyed by (image, cell), sorted stably, each cell summed in record order.  Every float is written,
 *   or with accumulate != 0 added to (layers/grad_fan.py: the map has other readers).
 *   workspace: jtsm_point_gather_backward_map_workspace_bytes(R, P, N, H, W).
 *
 * jtsm_point_select_f32 — `get_uncertain_point_coords_with_randomness` with `calculate_uncertainty`
 *   (point_features.py:72-125, mask_head.py:23-45).  coarse_logits (R, C, S, S) plain; classes (R) int64 (unused when
 *   C == 1); candidates (R, K, 2) and randoms (R, P - num_uncertain, 2) are the two torch.rand draws.  point_coords
 *   (R, P, 2) <- the num_uncertain candidates with the largest -|logit|, most uncertain first, EQUAL UNCERTAINTIES BY
 *   LOWER CANDIDATE INDEX, then the randoms.  chosen (R, num_uncertain) int32, optional: the candidates' indices.
 *
 * jtsm_point_loss_forward_f32 / _backward_f32 — `roi_mask_point_loss` (point_head.py:22-96).  logits (R * P, ld);
 *   `masks` is a HOST array of N (<= 64) device pointers to (count, h, w) uint8 / bool bitmasks and mask_geom a HOST
 *   array of N rows (h, w, count) int32; roi r reads mask matched[r] of image roi_image[r] at coords_wrt_image / (w, h).
 *   *loss <- mean over R * P of BCE-with-logits of the class column (column 0 when C == 1) against the soft target;
 *   stats[0] <- rows with (logit > 0) == uint8(target), stats[1] <- R * P.  R == 0 gives 0.  Sums are fp64 partials per
 *   workgroup folded in a fixed order.  workspace: jtsm_point_loss_workspace_bytes(R, P); it starts with the R * P soft
 *   targets and is carried to the backward, which writes every float of grad_logits (R * P, C; grad_ld apart).
 *
 * jtsm_point_subdivide_f32 — one step of `_forward_mask_point`'s loop (mask_head.py:245-261) on ONE channel: map
 *   (R, H, W) -> upsampled_map (R, 2H, 2W) by F.interpolate(scale_factor = 2, "bilinear"), and, when num_points > 0,
 *   `get_uncertain_point_coords_on_grid`: indices (R, n) int64 and point_coords (R, n, 2), n = min(4 H W, num_points),
 *   most uncertain first, EQUAL UNCERTAINTIES BY LOWER CELL INDEX.  H * W <= 12544, num_points <= 1024.
 * jtsm_point_topk_grid_f32 — `get_uncertain_point_coords_on_grid` (point_features.py:128-152) on a given (R, H, W)
 *   uncertainty map, read from memory: the num_points (<= min(H W, 1024)) largest values, same order and tie rule.
 * jtsm_point_scatter_f32 — map[r, indices[r, j]] <- point_logits[r * n + j, classes[r]] (column 0 when C == 1).
 * ------------------------------------------------------------------------------------------------------------------ */
int jtsm_point_gather_forward_f32(const float* const* maps, const int64_t* geom, const float* scales, int L,
                                  int num_images, const float* boxes, const int32_t* roi_image, const float* points,
                                  int R, int P, int grid_side, int space_to_depth, float* rows, int64_t row_stride,
                                  float* coords_wrt_image, void* stream);
int jtsm_point_gather_backward_roi_f32(const float* grad_rows, int64_t row_stride, int col, const float* points, int R,
                                       int P, int grid_side, int space_to_depth, int C, int H, int W, float* grad_map,
                                       int64_t stride_n, int64_t stride_c, int64_t stride_y, int64_t stride_x,
                                       void* stream);
size_t jtsm_point_gather_backward_map_workspace_bytes(int R, int P, int N, int H, int W);
int jtsm_point_gather_backward_map_f32(const float* grad_rows, int64_t row_stride, int col, const float* boxes,
                                       const int32_t* roi_image, const float* points, int R, int P, int grid_side,
                                       int space_to_depth, int N, int H, int W, int C, float scale, float* grad_map,
                                       int accumulate, void* workspace, size_t workspace_bytes, void* stream);
int jtsm_point_select_f32(const float* coarse_logits, int R, int C, int S, const int64_t* classes,
                          const float* candidates, int num_candidates, const float* randoms, int num_uncertain,
                          int P, float* point_coords, int32_t* chosen, void* stream);
size_t jtsm_point_loss_workspace_bytes(int R, int P);
int jtsm_point_loss_forward_f32(const float* logits, int64_t ld, int R, int P, int C, const int64_t* classes,
                                const uint8_t* const* masks, const int32_t* mask_geom, int N, const int32_t* roi_image,
                                const int32_t* matched, const float* coords_wrt_image, float* loss, int32_t* stats,
                                void* workspace, void* stream);
int jtsm_point_loss_backward_f32(const float* logits, int64_t ld, int R, int P, int C, const int64_t* classes,
                                 const float* grad_loss, const void* workspace, float* grad_logits, int64_t grad_ld,
                                 void* stream);
int jtsm_point_subdivide_f32(const float* map, int R, int H, int W, float* upsampled_map, int num_points,
                             int64_t* indices, float* point_coords, void* stream);
int jtsm_point_topk_grid_f32(const float* uncertainty_map, int R, int H, int W, int num_points, int64_t* indices,
                             float* point_coords, void* stream);
int jtsm_point_scatter_f32(const float* point_logits, int64_t ld, int R, int num_points, int C, const int64_t* classes,
                           const int64_t* indices, int cells, float* map, void* stream);

/* Model input boundary: GeneralizedMCNNWSL.preprocess_image
 * (projects/WSL/wsl/modeling/meta_arch/mcnn.py:303-318) + ImageList.from_tensors
 * (detectron2/structures/image_list.py:71-125) in one launch: images[b] is the mapper's uint8 (C, h_b, w_b) planar
 * image on the device (`images`, `heights`, `widths`, `mean`, `stdv` are HOST arrays); out (B, Hp, Wp, C) float32
 * channels-last <- (x - mean[c]) / stdv[c] inside the image, pad_value in the bottom / right padding. */
int jtsm_preprocess_images_u8(const uint8_t* const* images, const int32_t* heights, const int32_t* widths, int B,
                              int C, const float* mean, const float* stdv, float pad_value, int Hp, int Wp,
                              float* out, void* stream);
/* The same for images that arrive as float32 planes (the reference accepts any dtype: `(x - mean) / std` promotes). */
int jtsm_preprocess_images_f32(const float* const* images, const int32_t* heights, const int32_t* widths, int B,
                               int C, const float* mean, const float* stdv, float pad_value, int Hp, int Wp,
                               float* out, void* stream);

/* ---------------------------------------------------------------------------
 * Panoptic-DeepLab (projects/Panoptic-DeepLab/panoptic_deeplab/panoptic_seg.py:536-561 center_losses / offset_losses,
 * post_processing.py:9-234 find_instance_center / group_pixels / merge_semantic_and_instance /
 * get_panoptic_segmentation, panoptic_seg.py:163-207 the instance rows; train_net.py:100-124 Adam).  DESIGN §4o.
 *
 * Losses: pred (N,Hs,Ws,ld) NHWC rows of which channels 0 .. C-1 are read (C = 1 centre, C = 2 offset), target
 * (N,C,Hs*S,Ws*S) planar, weights (N,Hs*S,Ws*S); up = bilinear xS, align_corners = False, never materialised.
 * kind 0: out[0] = sum((up - t)^2 * w) / sum(w); kind 1: out[0] = sum(|S * up - t| * w) / sum(w), the sum over both
 * channels and sum(w) counting a pixel once.  out[1] = 1 / sum(w).  sum(w) <= 0: out = {0, 0} and a zero gradient.  fp64
 * sums in a fixed order.  backward: dpred (N,Hs,Ws,ld) = *upstream (1 if NULL) * d out[0] / d pred, pad lanes zero; a
 * gather per source pixel; coefficients 2 (up - t) w / sum(w) and S sign(S up - t) w / sum(w), sign(0) = 0. */
size_t jtsm_pdl_loss_workspace_bytes(void);
int jtsm_pdl_loss_forward_f32(const float* pred, int ld, int C, const float* target, const float* weights, int kind,
                              float* out, void* workspace, int N, int Hs, int Ws, int S, void* stream);
int jtsm_pdl_loss_backward_f32(const float* pred, int ld, int C, const float* target, const float* weights, int kind,
                               const float* out, const float* upstream, float* dpred, int N, int Hs, int Ws, int S,
                               void* stream);
/* find_instance_center: x > threshold else -1; pixels that differ from their nms_kernel x nms_kernel maximum (odd,
 * <= 31, padded as F.max_pool2d) become -1; v = the top_k-th largest value of that map over all H*W pixels; centers
 * (top_k,2) int32 (y, x) <- the pixels strictly above max(v, 0) in row-major order (at most top_k - 1; unused rows -1),
 * *count <- their number.  1 <= top_k <= H*W. */
size_t jtsm_pdl_centers_workspace_bytes(int H, int W);
int jtsm_pdl_find_centers_f32(const float* heat, int H, int W, float threshold, int nms_kernel, int top_k,
                              int32_t* centers, int32_t* count, void* workspace, void* stream);
/* sem (H,W) int32 <- arg-max over the C planes of logits (C,H,W), the first maximum. */
int jtsm_pdl_argmax_f32(const float* logits, int C, int H, int W, int32_t* sem, void* stream);
/* group_pixels: ins (H,W) int32 <- 1 + arg-min over the first min(*count, max_centers) centres of
 * sqrtf(dy*dy + dx*dx), dy = cy - (y + offsets[0,y,x]), dx = cx - (x + offsets[1,y,x]) in fp32, the lowest index on
 * equal distances; 0 where sem != NULL and thing_lut[sem] == 0 (thing_lut: num_classes bytes), and everywhere when
 * there is no centre.  max_centers <= 1024. */
int jtsm_pdl_group_pixels_f32(const int32_t* centers, const int32_t* count, int max_centers, const float* offsets,
                              const int32_t* sem, const uint8_t* thing_lut, int num_classes, int32_t* ins, int H, int W,
                              void* stream);
/* merge_semantic_and_instance with the segment table.  sem, ins (H,W) int32, ins in [0, max_instances]; a pixel is a
 * thing pixel where ins > 0 and (thing_seg != NULL ? thing_seg[p] : thing_lut[sem[p]]).  Per instance the majority
 * class (the smallest on equal counts); ids per class from 1 in ascending instance order, instances without a pixel
 * skipped; pan (H,W) int32 <- class * label_divisor + id on thing pixels, class * label_divisor on pixels with ins == 0
 * of a class with thing_lut == 0 and at least max(stuff_area, 1) such pixels, void_label elsewhere; id_offset is added
 * to every value; a class with label_divisor or more instances runs into the next class's ids, as in the reference.
 * table (max_instances + num_classes, 5) int32 rows {id, isthing, category, instance_id (-1: stuff),
 * area}: things in ascending instance order, then stuff in ascending class order; num[0] = rows, num[1] = thing rows.
 * logits (C,H,W), heat (H,W), inst (max_instances, 8) float, all three or none: per thing row {x0, y0, x1 + 1, y1 + 1,
 * mean soft-max probability of its class, heat at the truncated mean pixel, that pixel's y, x}. */
size_t jtsm_pdl_merge_workspace_bytes(int max_instances, int num_classes);
int jtsm_pdl_merge_f32(const int32_t* sem, const int32_t* ins, const uint8_t* thing_seg, const uint8_t* thing_lut,
                       const float* logits, const float* heat, int max_instances, int num_classes, int H, int W,
                       int label_divisor, int stuff_area, int void_label, int id_offset, int32_t* pan, int32_t* table,
                       int32_t* num, float* inst, void* workspace, void* stream);
/* torch.optim.Adam (weight decay added to the gradient, no amsgrad) over many tensors in ONE launch:
 * g += wd * p; m += (1 - b1) (g - m); v = b2 v + (1 - b2) g g; p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps).
 * table: `entries` records of ten 64-bit words {param, grad, exp_avg, exp_avg_sq, n, first_block, and four words of
 * two float bit patterns (low, high): (weight_decay, 1 - beta1), (beta2, 1 - beta2), (eps, lr / bias_correction1),
 * (sqrt(bias_correction2), 0)}; a record owns ceil(n / jtsm_adam_block_elements()) consecutive workgroups,
 * first_block is the running sum, `blocks` the total. */
int jtsm_adam_block_elements(void);
int jtsm_adam_multi_f32(const void* table, int entries, long blocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* JTSM_HIP_H_ */
