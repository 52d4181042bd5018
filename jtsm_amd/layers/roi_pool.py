"""ROIPool — Python surface of torchvision.ops.RoIPool as projects/WSL/wsl/modeling/poolers.py:6,183-186 uses it, on
top of libjtsm_hip.so (jtsm_roi_pool_{forward,backward}_f32; the contract is spelled out in csrc/roi_pool.hip).

forward(input (B,C,H,W), rois (R,5)) -> (R, C, PH, PW).  The output follows the input's memory format (channels_last
in, channels_last out).  float16 tensors are widened to float32 here and the result rounded back; max pooling only
selects values, so that is exact.

This file holds the one implementation of the library's ROI max pools.  An operator is a `MaxPoolOp`: its name, the
number of row blocks its output has per roi (ROIPool 1, ROILoopPool 3: layers/roi_loop_pool.py) and its three entry
points.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair

from .. import _lib as L
from .roi_align import _as_layout, _empty_like_layout

CL = torch.channels_last


class MaxPoolOp(object):
    def __init__(self, name, blocks, forward_sym, workspace_sym, backward_sym):
        self.name, self.blocks = name, blocks
        self.forward_sym, self.workspace_sym, self.backward_sym = forward_sym, workspace_sym, backward_sym

    def forward(self, input, rois, spatial_scale, pooled_h, pooled_w):
        """(output, argmax int32), both (blocks * R, C, PH, PW) in the input's memory format."""
        L.require_gpu(input, rois)
        if input.dtype not in (torch.float32, torch.float16):
            raise RuntimeError('"%s_forward" is implemented for float32 and float16, got %s' % (self.name, input.dtype))
        if input.dtype != rois.dtype:
            raise RuntimeError("expected input and rois to have the same dtype")
        if rois.dim() != 2 or rois.shape[1] != 5:
            raise RuntimeError("rois must be (R, 5), got %s" % (tuple(rois.shape),))
        half = input.dtype == torch.float16
        x, layout = _as_layout(input.float() if half else input)
        if half and layout == L.NHWC:
            x = x.contiguous(memory_format=CL)
        r = rois.float().contiguous()
        B, Cc, H, W = x.shape
        R = r.shape[0]
        out = _empty_like_layout((self.blocks * R, Cc, pooled_h, pooled_w), x, layout)
        fmt = CL if layout == L.NHWC else torch.contiguous_format
        arg = torch.empty((self.blocks * R, Cc, pooled_h, pooled_w), dtype=torch.int32, device=x.device,
                          memory_format=fmt)
        if out.numel():
            L.note_bytes(4.0 * (2 * out.numel() + r.numel()))
            L.check(getattr(L.lib(), self.forward_sym)(
                L.ptr(x), L.ptr(r), L.ptr(out), L.ptr(arg), B, Cc, H, W, R, spatial_scale, pooled_h, pooled_w,
                layout, L.stream()), self.forward_sym[5:-4])
        if half:
            out = out.half()
        return out, arg

    def backward(self, grad, rois, argmax, spatial_scale, pooled_h, pooled_w, B, Cc, H, W, nhwc=None):
        """grad_input (B, C, H, W) in the forward input's memory format (`nhwc`; None: read from `argmax`), dtype of
        `grad`.  The kernel reads and writes channels_last; NCHW tensors are converted at this boundary."""
        L.require_gpu(grad, rois, argmax)
        nchw = (not nhwc) if nhwc is not None else (not L.is_nhwc(argmax) and argmax.numel() > 0 and argmax.shape[1] > 1)
        half = grad.dtype == torch.float16
        g = (grad.float() if half else grad).contiguous(memory_format=CL)
        a = argmax.contiguous(memory_format=CL)
        r = rois.float().contiguous()
        gin = torch.empty((B, Cc, H, W), dtype=torch.float32, device=g.device, memory_format=CL)
        if gin.numel():
            lib = L.lib()
            ws = torch.empty(max(getattr(lib, self.workspace_sym)(r.shape[0]), 16), dtype=torch.uint8, device=g.device)
            L.note_bytes(4.0 * (2 * g.numel() + gin.numel()))
            L.check(getattr(lib, self.backward_sym)(
                L.ptr(g), L.ptr(r), L.ptr(a), L.ptr(gin), L.ptr(ws), B, Cc, H, W, r.shape[0], spatial_scale,
                pooled_h, pooled_w, L.stream()), self.backward_sym[5:-4])
        if nchw:
            gin = gin.contiguous()
        return gin.half() if half else gin

    def apply(self, input, roi, output_size, spatial_scale):
        return _MaxPool.apply(self, input, roi, output_size, spatial_scale)


class _MaxPool(Function):
    @staticmethod
    def forward(ctx, op, input, roi, output_size, spatial_scale):
        ctx.op = op
        ctx.output_size = _pair(output_size)
        ctx.spatial_scale = spatial_scale
        ctx.input_shape = input.size()
        ctx.nhwc = L.is_nhwc(input)
        output, argmax = op.forward(input, roi, spatial_scale, ctx.output_size[0], ctx.output_size[1])
        ctx.save_for_backward(roi, argmax)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        rois, argmax = ctx.saved_tensors
        bs, ch, h, w = ctx.input_shape
        grad_input = ctx.op.backward(grad_output, rois, argmax, ctx.spatial_scale, ctx.output_size[0],
                                     ctx.output_size[1], bs, ch, h, w, nhwc=ctx.nhwc)
        return None, grad_input, None, None, None


class MaxPoolModule(nn.Module):
    """Module of the operator its subclass names in `op`."""
    op = None

    def __init__(self, output_size, spatial_scale):
        """output_size (h, w); spatial_scale: multiply boxes by this before rounding."""
        super().__init__()
        self.output_size = output_size
        self.spatial_scale = spatial_scale

    def forward(self, input, rois):
        """
        Args:
            input: NCHW features (channels_last storage is kept)
            rois: Rx5 boxes (batch index, x0, y0, x1, y1)
        Returns: (op.blocks * R, C, PH, PW)
        """
        assert rois.dim() == 2 and rois.size(1) == 5
        return self.op.apply(input, rois, self.output_size, self.spatial_scale)

    def __repr__(self):
        tmpstr = self.__class__.__name__ + "("
        tmpstr += "output_size=" + str(self.output_size)
        tmpstr += ", spatial_scale=" + str(self.spatial_scale)
        tmpstr += ")"
        return tmpstr


_OP = MaxPoolOp("ROIPool", 1, "jtsm_roi_pool_forward_f32", "jtsm_roi_pool_backward_workspace_bytes",
                "jtsm_roi_pool_backward_f32")
roi_pool_forward, roi_pool_backward, roi_pool = _OP.forward, _OP.backward, _OP.apply


class ROIPool(MaxPoolModule):
    op = _OP
