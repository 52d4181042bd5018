"""DeformConv / ModulatedDeformConv — surface of detectron2/layers/deform_conv.py (constructor arguments, parameter
names, extra_repr), on this package's own kernels.

One autograd node serves v1 and v2 (the mask is optional).  Forward: the sampled columns (csrc/deform_conv.hip) as a
(N * Ho * Wo) x (kh * kw * C) matrix, tap-major and channel-minor — the order in which a channels-last (O, C, kh, kw)
weight already lies — then the package's ordinary contraction as a 1x1 convolution over that matrix, with FrozenBN
scale / bias, the bias and the ReLU in its epilogue (as wrappers.Conv2d folds them).  Backward: the columns are
recomputed (the reference does not keep them either); conv2d_backward_data gives their gradient, conv2d_backward_weight
the weight's (and the bias's), the offset / mask kernel and the sorted input-gradient gather the rest.  Every
JTSM_CONV_MATH arithmetic works because the contraction is the existing one; the columns are fp32 and are split by it.
The weight gradient is returned to autograd (not written into the data-parallel buckets).
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair

from .. import _lib as L
from . import conv
from .batch_norm import FrozenBatchNorm2d
from .conv import CL

# The whole batch's columns above this many bytes: forward and backward loop over groups of images.
MAX_COLUMN_BYTES = 256 << 20


def _square(v, what):
    a, b = _pair(v)
    if a != b:
        raise NotImplementedError("jtsm_amd deformable conv: square %s only, got %s" % (what, (a, b)))
    return int(a)


def _out_hw(h, w, kh, kw, stride, pad, dil):
    return ((h + 2 * pad - dil * (kh - 1) - 1) // stride + 1, (w + 2 * pad - dil * (kw - 1) - 1) // stride + 1)


def _dims(x, kh, kw, stride, pad, dil, G):
    n, c, h, w = x.shape
    return (n, h, w, c, G, kh, kw, stride, pad, dil)


def _nhwc_like(t):
    """A fresh tensor of t's logical shape in channels-last memory."""
    return torch.empty(t.shape, dtype=t.dtype, device=t.device, memory_format=CL)


def deform_columns(x, offset, mask, kh, kw, stride, pad, dil, G, out=None):
    """The sampled columns of x (N, C, H, W) as a logical (N, kh * kw * C, Ho, Wo) channels-last tensor: row (n, oy, ox)
    holds tap-major, channel-minor samples.  offset (N, G * 2 * kh * kw, Ho, Wo), mask (N, G * kh * kw, Ho, Wo) or None."""
    L.require_gpu(x, offset, mask)
    x, offset = conv._cl(x), conv._cl(offset)
    mask = conv._cl(mask) if mask is not None else None
    n, c, h, w = x.shape
    ho, wo = offset.shape[2:]
    if out is None:
        out = torch.empty((n, kh * kw * c, ho, wo), dtype=x.dtype, device=x.device, memory_format=CL)
    L.note_bytes(4.0 * (out.numel() * 2 + offset.numel()))
    L.check(L.lib().jtsm_deform_columns_f32(L.ptr(x), L.ptr(offset), L.ptr(mask), L.ptr(out),
                                            *_dims(x, kh, kw, stride, pad, dil, G), L.stream()), "deform_columns")
    return out


def deform_offset_mask_grad(dcols, x, offset, mask, kh, kw, stride, pad, dil, G):
    """(d_offset, d_mask or None) in offset's / mask's shape from the columns' gradient (deform_columns' layout)."""
    L.require_gpu(dcols, x, offset, mask)
    dcols, x, offset = conv._cl(dcols), conv._cl(x), conv._cl(offset)
    mask = conv._cl(mask) if mask is not None else None
    d_offset = _nhwc_like(offset)
    d_mask = _nhwc_like(mask) if mask is not None else None
    L.note_bytes(4.0 * (dcols.numel() * 2 + offset.numel() * 3))
    L.check(L.lib().jtsm_deform_offset_mask_grad_f32(
        L.ptr(dcols), L.ptr(x), L.ptr(offset), L.ptr(mask), L.ptr(d_offset), L.ptr(d_mask),
        *_dims(x, kh, kw, stride, pad, dil, G), L.stream()), "deform_offset_mask_grad")
    return d_offset, d_mask


def deform_input_grad(dcols, offset, mask, x_shape, kh, kw, stride, pad, dil, G):
    """dx (x_shape, channels-last) from the columns' gradient: the sorted, deterministic gather."""
    L.require_gpu(dcols, offset, mask)
    dcols, offset = conv._cl(dcols), conv._cl(offset)
    mask = conv._cl(mask) if mask is not None else None
    n, c, h, w = x_shape
    dx = torch.empty(tuple(x_shape), dtype=dcols.dtype, device=dcols.device, memory_format=CL)   # every element is written
    lib = L.lib()
    nbytes = lib.jtsm_deform_input_grad_workspace_bytes(n, h, w, G, kh, kw, stride, pad, dil)
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dcols.device)
    ws = ws[(-ws.data_ptr()) % 256:]
    L.note_bytes(4.0 * (dcols.numel() + dx.numel()))
    L.check(lib.jtsm_deform_input_grad_f32(L.ptr(dcols), L.ptr(offset), L.ptr(mask), L.ptr(dx), n, h, w, c, G, kh, kw,
                                           stride, pad, dil, L.ptr(ws), nbytes, L.stream()), "deform_input_grad")
    return dx


def _column_buffer(n, kc, ho, wo, reserve, device):
    """The (n, kc, ho, wo) channels-last column matrix inside conv._scratch, behind the `reserve` bytes the contractions
    over it take from the front of the same buffer for their split-K slabs."""
    front = (reserve + 255) & ~255
    nbytes = 4 * n * kc * ho * wo
    buf = conv._scratch(front + nbytes + 256, device)
    front += (-(buf.data_ptr() + front)) % 256
    cols = buf[front:front + nbytes].view(torch.float32).view(n, ho, wo, kc).permute(0, 3, 1, 2)
    return cols


def _image_groups(n, bytes_per_image):
    step = max(1, min(n, MAX_COLUMN_BYTES // max(bytes_per_image, 1)))
    return [(a, min(n, a + step)) for a in range(0, n, step)]


def _check_shapes(x, offset, mask, weight, stride, pad, dil, G):
    if x.dim() != 4:
        raise ValueError("Expected 4D tensor as input, got {}D tensor instead.".format(x.dim()))
    o, ci, kh, kw = weight.shape
    n, c, h, w = x.shape
    if ci != c:
        raise NotImplementedError("jtsm_amd deformable conv: groups=1 only (weight has %d input channels, x has %d)"
                                  % (ci, c))
    ho, wo = _out_hw(h, w, kh, kw, stride, pad, dil)
    if n > 0 and (ho <= 0 or wo <= 0):
        raise ValueError("convolution input is too small (output would be {})".format("x".join(map(str, (n, o, ho, wo)))))
    want = (n, G * 2 * kh * kw, ho, wo)
    if tuple(offset.shape) != want:
        raise ValueError("deformable conv: offset has shape %s, expected %s" % (tuple(offset.shape), want))
    if mask is not None:
        want = (n, G * kh * kw, ho, wo)
        if tuple(mask.shape) != want:
            raise ValueError("deformable conv: mask has shape %s, expected %s" % (tuple(mask.shape), want))
    return ho, wo


class _DeformConvFn(Function):
    """y = relu?(deform_conv(x, offset, mask, w) * scale + bias): scale is a constant of the op (FrozenBN), bias gets its
    gradient when it asks for one (ModulatedDeformConv's own bias, alone or folded into the FrozenBN shift)."""

    @staticmethod
    def forward(ctx, x, offset, mask, weight, scale, bias, stride, pad, dil, G, relu):
        conv._check(x, offset, mask, weight, scale, bias)
        x, offset, weight = conv._cl(x), conv._cl(offset), conv._cl(weight)
        mask = conv._cl(mask) if mask is not None else None
        o, c, kh, kw = weight.shape
        n, _, h, w = x.shape
        ho, wo = offset.shape[2:]
        kc = kh * kw * c
        w2 = weight.permute(0, 2, 3, 1).reshape(o, kc, 1, 1)     # (O, kh, kw, C) rows: the same bytes, no repacking
        ys = []
        for a, b in _image_groups(n, 4 * kc * ho * wo):
            pl = conv._plan((b - a, kc, ho, wo), w2.shape, 1, 0, 1)
            cols = _column_buffer(b - a, kc, ho, wo, pl.ws[0], x.device)
            deform_columns(x[a:b], offset[a:b], mask[a:b] if mask is not None else None, kh, kw, stride, pad, dil, G,
                           out=cols)
            conv.planes_forget(cols)      # (the buffer is reused: planes cached for these bytes are another call's)
            ys.append(conv.conv2d_forward(cols, w2, 1, 0, 1, scale, bias, None, relu))
            conv.planes_forget(cols)
        y = ys[0] if len(ys) == 1 else torch.cat(ys).contiguous(memory_format=CL)
        ctx.cfg = (stride, pad, dil, G, relu, kh, kw)
        ctx.save_for_backward(x, offset, mask, weight, scale, y if relu else None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        from .elementwise import channel_sum, relu_backward

        x, offset, mask, weight, scale, y = ctx.saved_tensors
        stride, pad, dil, G, relu, kh, kw = ctx.cfg
        g = relu_backward(dy, y) if relu else conv._cl(dy)
        o, c = weight.shape[:2]
        n, _, h, w = x.shape
        ho, wo = offset.shape[2:]
        kc = kh * kw * c
        w2 = weight.permute(0, 2, 3, 1).reshape(o, kc, 1, 1)
        need_x, need_off, need_mask, need_w = ctx.needs_input_grad[:4]
        need_mask = need_mask and mask is not None
        want_db = ctx.needs_input_grad[5]
        db_in_wgrad = want_db and scale is None      # (the contraction's bias sum rides beside an unscaled dw only)
        need_dcols = need_x or need_off or need_mask
        w_eff = w2
        if need_dcols and scale is not None and conv.MATH == "f32":
            w_eff = (w2 * scale.view(-1, 1, 1, 1)).contiguous(memory_format=CL)
        dxs, doffs, dmasks, dw, db = [], [], [], None, None
        for a, b in _image_groups(n, 4 * kc * ho * wo):
            xs, offs, gs = x[a:b], offset[a:b], g[a:b]
            ms = mask[a:b] if mask is not None else None
            shape = (b - a, kc, ho, wo)
            if need_dcols:
                if conv.MATH != "f32":
                    dcols = conv.conv2d_backward_data(gs, w2, shape, 1, 0, 1, kscale=scale)
                else:
                    dcols = conv.conv2d_backward_data(gs, w_eff, shape, 1, 0, 1)
                if need_off or need_mask:
                    d_off, d_m = deform_offset_mask_grad(dcols, xs, offs, ms, kh, kw, stride, pad, dil, G)
                    doffs.append(d_off)
                    dmasks.append(d_m)
                if need_x:
                    dxs.append(deform_input_grad(dcols, offs, ms, xs.shape, kh, kw, stride, pad, dil, G))
                del dcols
            if need_w:
                pl = conv._plan(shape, w2.shape, 1, 0, 1)
                # (where the bias sum does not ride in the contraction, conv2d_backward_weight takes it by channel_sum,
                # whose partials come from the front of the same scratch)
                reserve = max(max(pl.ws), L.lib().jtsm_channel_sum_workspace_bytes((b - a) * ho * wo, o) if db_in_wgrad else 0)
                cols = _column_buffer(b - a, kc, ho, wo, reserve, x.device)
                deform_columns(xs, offs, ms, kh, kw, stride, pad, dil, G, out=cols)
                conv.planes_forget(cols)
                db_ = torch.empty(o, dtype=g.dtype, device=g.device) if db_in_wgrad else None
                dw_ = conv.conv2d_backward_weight(gs, cols, w2.shape, 1, 0, 1, row_scale=scale, bias_out=db_)
                conv.planes_forget(cols)
                dw = dw_ if dw is None else dw + dw_      # (groups of images: fresh results, summed in order)
                if db_in_wgrad:
                    db = db_ if db is None else db + db_
        if want_db and db is None:
            db = channel_sum(g)

        def join(parts):
            if not parts or parts[0] is None:
                return None
            return parts[0] if len(parts) == 1 else torch.cat(parts).contiguous(memory_format=CL)

        if dw is not None:      # (O, kh * kw * C) rows back as the channels-last (O, C, kh, kw) they are
            dw = dw.reshape(o, kh, kw, c).permute(0, 3, 1, 2)
        return (join(dxs) if need_x else None, join(doffs) if need_off else None, join(dmasks) if need_mask else None,
                dw, None, db, None, None, None, None, None)


def _apply(x, offset, mask, weight, bias, stride, padding, dilation, groups, deformable_groups, scale=None,
           shift=None, relu=False):
    if groups != 1:
        raise NotImplementedError("jtsm_amd deformable conv: groups=1 only, got groups=%d" % groups)
    stride, pad, dil = _square(stride, "stride"), _square(padding, "padding"), _square(dilation, "dilation")
    L.require_gpu(x, offset, mask, weight, bias)
    ho, wo = _check_shapes(x, offset, mask, weight, stride, pad, dil, deformable_groups)
    if x.shape[0] == 0:
        return x.new_empty((0, weight.shape[0], max(ho, 0), max(wo, 0)))
    if scale is not None:       # FrozenBN: y * scale + shift, a bias rides inside the shift
        bias = shift if bias is None else shift + bias * scale
    return _DeformConvFn.apply(x, offset, mask, weight, scale, bias, stride, pad, dil, deformable_groups, relu)


def deform_conv(input, offset, weight, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, im2col_step=64):
    """Deformable convolution v1 (deform_conv.py:16-183; im2col_step is accepted and has no meaning here)."""
    return _apply(input, offset, None, weight, None, stride, padding, dilation, groups, deformable_groups)


def modulated_deform_conv(input, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, groups=1,
                          deformable_groups=1):
    """Deformable convolution v2 (deform_conv.py:186-308)."""
    return _apply(input, offset, mask, weight, bias, stride, padding, dilation, groups, deformable_groups)


class _DeformBase(nn.Module):
    def _init(self, in_channels, out_channels, kernel_size, groups, bias):
        if groups != 1:
            raise NotImplementedError("jtsm_amd deformable conv: groups=1 only, got groups=%d" % groups)
        for v, what in ((self.stride, "stride"), (self.padding, "padding"), (self.dilation, "dilation")):
            _square(v, what)
        # OHWI storage: what the kernels read; the logical shape stays (O, I, kh, kw)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, *self.kernel_size)
                                   .contiguous(memory_format=CL))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        nn.init.kaiming_uniform_(self.weight, nonlinearity="relu")
        if self.bias is not None:
            nn.init.constant_(self.bias, 0)

    def _run(self, x, offset, mask):
        from .wrappers import _is_relu

        fuse_norm = isinstance(self.norm, FrozenBatchNorm2d)
        relu = _is_relu(self.activation) and (self.norm is None or fuse_norm)
        scale, shift = self.norm.scale_bias() if fuse_norm else (None, None)
        y = _apply(x, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation, self.groups,
                   self.deformable_groups, scale, shift, relu)
        if x.shape[0] == 0:
            return y
        if self.norm is not None and not fuse_norm:
            y = self.norm(y)
        if self.activation is not None and not relu:
            y = self.activation(y)
        return y

    def _repr(self, bias):
        tmpstr = "in_channels=" + str(self.in_channels)
        tmpstr += ", out_channels=" + str(self.out_channels)
        tmpstr += ", kernel_size=" + str(self.kernel_size)
        tmpstr += ", stride=" + str(self.stride)
        tmpstr += ", padding=" + str(self.padding)
        tmpstr += ", dilation=" + str(self.dilation)
        tmpstr += ", groups=" + str(self.groups)
        tmpstr += ", deformable_groups=" + str(self.deformable_groups)
        tmpstr += ", bias=" + bias
        return tmpstr


class DeformConv(_DeformBase):
    """Deformable convolution v1 (deform_conv.py:315-409): forward(x, offset)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 deformable_groups=1, bias=False, norm=None, activation=None):
        super().__init__()
        assert not bias
        assert in_channels % groups == 0, "in_channels {} cannot be divisible by groups {}".format(in_channels, groups)
        assert out_channels % groups == 0, "out_channels {} cannot be divisible by groups {}".format(out_channels, groups)
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = _pair(kernel_size)
        self.stride = _pair(stride)
        self.padding = _pair(padding)
        self.dilation = _pair(dilation)
        self.groups = groups
        self.deformable_groups = deformable_groups
        self.norm = norm
        self.activation = activation
        self._init(in_channels, out_channels, kernel_size, groups, False)

    def forward(self, x, offset):
        return self._run(x, offset, None)

    def extra_repr(self):
        return self._repr("False")


class ModulatedDeformConv(_DeformBase):
    """Deformable convolution v2 (deform_conv.py:412-501): forward(x, offset, mask)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 deformable_groups=1, bias=True, norm=None, activation=None):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = _pair(kernel_size)
        self.stride = stride
        self.padding = padding
        self.dilation = dilation
        self.groups = groups
        self.deformable_groups = deformable_groups
        self.with_bias = bias
        self.norm = norm
        self.activation = activation
        self._init(in_channels, out_channels, kernel_size, groups, bias)

    def forward(self, x, offset, mask):
        return self._run(x, offset, mask)

    def extra_repr(self):
        return self._repr(str(self.with_bias))
