"""ASPP — constructor, module names (convs.0 .. convs.4, project; convs.4.1 the biased 1x1 behind the image pooling)
and forward of detectron2/layers/aspp.py:14-144.

MI355X mapping: the 1x1 and the three dilated 3x3 branches are contraction launches (layers/conv.py takes any dilation)
each followed by the fused norm + ReLU pass (csrc/batch_norm.hip); with `pool_kernel_size` equal to the map — the
training crop — the image pooling is a per-(image, channel) mean (the statistics reduction of the same file) and its
"up-sampling" a broadcast: bilinear interpolation of a 1x1 map copies it.  On a larger map (inference on whole images)
the pooling window slides: torch's avg_pool2d and the library's bilinear resize."""
import torch
import torch.nn.functional as F
from torch import nn

from .batch_norm import get_norm, image_mean
from .wrappers import Conv2d

CL = torch.channels_last


def c2_xavier_fill(module):
    """fvcore's c2_xavier_fill (not in the reference tree): kaiming_uniform(a=1), zero bias."""
    nn.init.kaiming_uniform_(module.weight, a=1)
    if module.bias is not None:
        nn.init.constant_(module.bias, 0)


class _ImagePool(nn.Module):
    """Stands where the reference has nn.AdaptiveAvgPool2d(1) / nn.AvgPool2d(pool_kernel_size, stride=1): no state."""

    def __init__(self, kernel_size):
        super().__init__()
        self.kernel_size = kernel_size

    def forward(self, x):
        size = tuple(x.shape[-2:])
        if self.kernel_size is None or tuple(self.kernel_size) == size:
            return image_mean(x) if x.is_cuda else F.adaptive_avg_pool2d(x, 1)
        return F.avg_pool2d(x, kernel_size=tuple(self.kernel_size), stride=1)

    def extra_repr(self):
        return "kernel_size=%s" % (self.kernel_size,)


def broadcast_or_resize(pooled, size):
    """F.interpolate(pooled, size=size, mode="bilinear", align_corners=False): a broadcast for a 1x1 map (bit for bit
    what the interpolation gives), otherwise the library's resize (inference) or torch's (under autograd)."""
    if tuple(pooled.shape[-2:]) == (1, 1):
        return pooled.expand(-1, -1, size[0], size[1])
    if pooled.is_cuda and not (torch.is_grad_enabled() and pooled.requires_grad):
        from .postprocess import resize_bilinear
        return resize_bilinear(pooled, size).contiguous(memory_format=CL)
    return F.interpolate(pooled, size=size, mode="bilinear", align_corners=False)


class ASPP(nn.Module):
    def __init__(self, in_channels, out_channels, dilations, *, norm, activation, pool_kernel_size=None,
                 dropout: float = 0.0, use_depthwise_separable_conv=False):
        super().__init__()
        assert len(dilations) == 3, "ASPP expects 3 dilations, got {}".format(len(dilations))
        if use_depthwise_separable_conv:
            raise NotImplementedError("jtsm_amd ASPP: use_depthwise_separable_conv is not built (no shipped DeepLab "
                                      "config sets it)")
        self.pool_kernel_size = pool_kernel_size
        self.dropout = dropout
        use_bias = norm == ""
        self.convs = nn.ModuleList()
        self.convs.append(Conv2d(in_channels, out_channels, kernel_size=1, bias=use_bias,
                                 norm=get_norm(norm, out_channels), activation=activation))
        for dilation in dilations:
            self.convs.append(Conv2d(in_channels, out_channels, kernel_size=3, padding=dilation, dilation=dilation,
                                     bias=use_bias, norm=get_norm(norm, out_channels), activation=activation))
        # no norm behind the image pooling: its map is 1x1 (aspp.py:103-105)
        self.convs.append(nn.Sequential(_ImagePool(pool_kernel_size),
                                        Conv2d(in_channels, out_channels, 1, bias=True, activation=activation)))
        self.project = Conv2d(5 * out_channels, out_channels, kernel_size=1, bias=use_bias,
                              norm=get_norm(norm, out_channels), activation=activation)
        for conv in list(self.convs[:4]) + [self.convs[4][1], self.project]:
            c2_xavier_fill(conv)

    def forward(self, x):
        size = tuple(x.shape[-2:])
        if self.pool_kernel_size is not None:
            if size[0] % self.pool_kernel_size[0] or size[1] % self.pool_kernel_size[1]:
                raise ValueError("`pool_kernel_size` must be divisible by the shape of inputs. "
                                 "Input size: {} `pool_kernel_size`: {}".format(size, self.pool_kernel_size))
        res = [conv(x) for conv in self.convs]
        res[-1] = broadcast_or_resize(res[-1], size)
        res = self.project(torch.cat(res, dim=1).contiguous(memory_format=CL))
        return F.dropout(res, self.dropout, training=self.training) if self.dropout > 0 else res
