"""DeepLabV3PlusHead / DeepLabV3Head — constructor keywords, from_config, module names (decoder.<feature>.project_conv /
.fuse_conv, aspp, predictor) and losses of projects/DeepLab/deeplab/semantic_seg.py:15-349.

MI355X mapping: every convolution is a contraction launch followed by the fused batch norm + ReLU pass
(layers/wrappers.py, csrc/batch_norm.hip); the decoder's up-sampling is the integer-scale bilinear kernel of
csrc/semseg_ops.hip with a gather backward (the same bits on every run; a ratio that is no integer is served in
evaluation mode only, by the library's resize); the loss never sees full-resolution logits: `cross_entropy` is
semseg_cross_entropy, `hard_pixel_mining` is deeplab_cross_entropy with the top 20 % (csrc/deeplab_loss.hip).
torch.cat and F.dropout are device-side torch glue."""
from typing import Callable, Dict, List, Optional, Tuple, Union

import torch
import torch.nn.functional as F
from torch import nn

from ...layers.aspp import ASPP, c2_xavier_fill
from ...layers.batch_norm import get_norm
from ...layers.shape_spec import ShapeSpec
from ...layers.wrappers import Conv2d, conv2d_padded
from .semantic_seg import SEM_SEG_HEADS_REGISTRY, _upsample_logits

CL = torch.channels_last
_LOSS_TYPES = ("cross_entropy", "hard_pixel_mining")


def _upsample_to(y, size):
    """F.interpolate(y, size=size, mode="bilinear", align_corners=False) on a channels_last map."""
    h, w = y.shape[-2:]
    if (h, w) == tuple(size):
        return y
    if not y.is_cuda:
        return F.interpolate(y, size=size, mode="bilinear", align_corners=False)
    if size[0] % h == 0 and size[1] % w == 0 and size[0] // h == size[1] // w:
        from ...layers.elementwise import upsample_bilinear
        return upsample_bilinear(y, size[0] // h)
    if torch.is_grad_enabled() and y.requires_grad:
        raise NotImplementedError("DeepLab decoder: training needs maps whose sizes are integer multiples of each other "
                                  "(got %s -> %s); crop to a multiple of the encoder stride" % ((h, w), tuple(size)))
    from ...layers.postprocess import resize_bilinear
    return resize_bilinear(y, size).contiguous(memory_format=CL)


def _segmentation_loss(predictions, targets, common_stride, ignore_value, loss_type, loss_weight, top_k=0.2,
                       weights=None):
    """`loss(F.interpolate(predictions, scale_factor=common_stride, "bilinear"), targets) * loss_weight`; `top_k` and the
    per-pixel `weights` are hard_pixel_mining's (DeepLabCE's top_k_percent_pixels and third argument)."""
    from ...layers.elementwise import deeplab_cross_entropy, semseg_cross_entropy
    if not (predictions.is_cuda and predictions.shape[1] <= 64 and common_stride == int(common_stride)):
        raise NotImplementedError("semantic loss: <= 64 classes, an integer stride, on the HIP device only")
    if loss_type == "cross_entropy":
        if weights is not None:            # (the reference's nn.CrossEntropyLoss takes no third argument either)
            raise ValueError("semantic loss: per-pixel weights need loss_type 'hard_pixel_mining', not 'cross_entropy'")
        loss = semseg_cross_entropy(predictions.float(), targets, int(common_stride), ignore_value)
    else:
        loss = deeplab_cross_entropy(predictions.float(), targets, int(common_stride), ignore_value, top_k,
                                     weights=weights)
    return {"loss_sem_seg": loss * loss_weight}


def _predictor(in_channels, num_classes):
    conv = Conv2d(in_channels, num_classes, kernel_size=1, stride=1, padding=0)
    nn.init.normal_(conv.weight, 0, 0.001)
    nn.init.constant_(conv.bias, 0)
    return conv


def _predict(conv, y):
    # (through conv2d_padded: a class count that is no multiple of 8 must still train to the same bits twice)
    return conv2d_padded(conv, y) if y.is_cuda else conv(y)


def _pool_kernel_size(train_size, stride, what):
    if train_size is None:
        return None
    train_h, train_w = train_size
    if train_h % stride or train_w % stride:
        raise ValueError("Crop size need to be divisible by %s." % what)
    return (train_h // stride, train_w // stride)


@SEM_SEG_HEADS_REGISTRY.register()
class DeepLabV3PlusHead(nn.Module):
    """DeepLabV3PlusHead(cfg, input_shape) or the reference's keyword constructor (`input_shape=..., in_features=...`)."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        if args and hasattr(args[0], "MODEL"):            # (cfg, input_shape): what the registry calls
            kwargs = dict(self.from_config(*args), **kwargs)
            args = ()
        self._build(*args, **kwargs)

    def _build(self, input_shape: Dict[str, ShapeSpec], *, in_features: List[str], project_channels: List[int],
               aspp_dilations: List[int], aspp_dropout: float, decoder_channels: List[int], common_stride: int,
               norm: Union[str, Callable], train_size: Optional[Tuple], loss_weight: float = 1.0,
               loss_type: str = "cross_entropy", ignore_value: int = -1, num_classes: Optional[int] = None,
               use_depthwise_separable_conv: bool = False):
        self.in_features = in_features                     # from the highest resolution ("res2") to the lowest ("res5")
        in_channels = [input_shape[f].channels for f in in_features]
        aspp_channels = decoder_channels[-1]
        self.ignore_value, self.common_stride = ignore_value, common_stride
        self.loss_weight, self.loss_type = loss_weight, loss_type
        self.decoder_only = num_classes is None
        self.use_depthwise_separable_conv = use_depthwise_separable_conv
        if use_depthwise_separable_conv:
            raise NotImplementedError("jtsm_amd DeepLabV3PlusHead: use_depthwise_separable_conv is not built (no shipped "
                                      "DeepLab config sets it)")
        assert len(project_channels) == len(in_features) - 1, \
            "Expected {} project_channels, got {}".format(len(in_features) - 1, len(project_channels))
        assert len(decoder_channels) == len(in_features), \
            "Expected {} decoder_channels, got {}".format(len(in_features), len(decoder_channels))
        self.decoder = nn.ModuleDict()
        use_bias = norm == ""
        for idx, in_channel in enumerate(in_channels):
            stage = nn.ModuleDict()
            if idx == len(in_features) - 1:
                pool = _pool_kernel_size(train_size, input_shape[in_features[-1]].stride, "encoder stride")
                project_conv = ASPP(in_channel, aspp_channels, aspp_dilations, norm=norm, activation=F.relu,
                                    pool_kernel_size=pool, dropout=aspp_dropout)
                fuse_conv = None
            else:
                project_conv = Conv2d(in_channel, project_channels[idx], kernel_size=1, bias=use_bias,
                                      norm=get_norm(norm, project_channels[idx]), activation=F.relu)
                c2_xavier_fill(project_conv)
                fuse_conv = nn.Sequential(
                    Conv2d(project_channels[idx] + decoder_channels[idx + 1], decoder_channels[idx], kernel_size=3,
                           padding=1, bias=use_bias, norm=get_norm(norm, decoder_channels[idx]), activation=F.relu),
                    Conv2d(decoder_channels[idx], decoder_channels[idx], kernel_size=3, padding=1, bias=use_bias,
                           norm=get_norm(norm, decoder_channels[idx]), activation=F.relu))
                c2_xavier_fill(fuse_conv[0])
                c2_xavier_fill(fuse_conv[1])
            stage["project_conv"] = project_conv
            stage["fuse_conv"] = fuse_conv
            self.decoder[in_features[idx]] = stage
        if not self.decoder_only:
            self.predictor = _predictor(decoder_channels[0], num_classes)
            if loss_type not in _LOSS_TYPES:
                raise ValueError("Unexpected loss type: %s" % loss_type)

    @classmethod
    def from_config(cls, cfg, input_shape):
        head = cfg.MODEL.SEM_SEG_HEAD
        train_size = None
        if cfg.INPUT.CROP.ENABLED:
            assert cfg.INPUT.CROP.TYPE == "absolute"
            train_size = cfg.INPUT.CROP.SIZE
        decoder_channels = [head.CONVS_DIM] * (len(head.IN_FEATURES) - 1) + [head.ASPP_CHANNELS]
        return dict(input_shape=input_shape, in_features=head.IN_FEATURES, project_channels=head.PROJECT_CHANNELS,
                    aspp_dilations=head.ASPP_DILATIONS, aspp_dropout=head.ASPP_DROPOUT,
                    decoder_channels=decoder_channels, common_stride=head.COMMON_STRIDE, norm=head.NORM,
                    train_size=train_size, loss_weight=head.LOSS_WEIGHT, loss_type=head.LOSS_TYPE,
                    ignore_value=head.IGNORE_VALUE, num_classes=head.NUM_CLASSES,
                    use_depthwise_separable_conv=head.USE_DEPTHWISE_SEPARABLE_CONV)

    def forward(self, features, targets=None):
        """Training: (None, losses); inference: ((N, C, H, W) logits, {}); decoder-only: the decoder's map."""
        y = self.layers(features)
        if self.decoder_only:
            return y
        if self.training:
            return None, self.losses(y, targets)
        return _upsample_logits(y, self.common_stride), {}

    def layers(self, features):
        for f in self.in_features[::-1]:                   # from the lowest resolution up
            stage = self.decoder[f]
            proj_x = stage["project_conv"](features[f])
            if stage["fuse_conv"] is None:                 # the ASPP stage
                y = proj_x
            else:
                y = _upsample_to(y, tuple(proj_x.shape[2:]))
                y = stage["fuse_conv"](torch.cat([proj_x, y], dim=1).contiguous(memory_format=CL))
        if not self.decoder_only:
            y = _predict(self.predictor, y)
        return y

    def losses(self, predictions, targets):
        return _segmentation_loss(predictions, targets, self.common_stride, self.ignore_value, self.loss_type,
                                  self.loss_weight)


@SEM_SEG_HEADS_REGISTRY.register()
class DeepLabV3Head(nn.Module):
    def __init__(self, cfg, input_shape: Dict[str, ShapeSpec]):
        super().__init__()
        head = cfg.MODEL.SEM_SEG_HEAD
        self.in_features = head.IN_FEATURES
        in_channels = [input_shape[f].channels for f in self.in_features]
        self.ignore_value, self.common_stride = head.IGNORE_VALUE, head.COMMON_STRIDE
        self.loss_weight, self.loss_type = head.LOSS_WEIGHT, head.LOSS_TYPE
        assert len(self.in_features) == 1
        assert len(in_channels) == 1
        pool = None
        if cfg.INPUT.CROP.ENABLED:
            assert cfg.INPUT.CROP.TYPE == "absolute"
            pool = _pool_kernel_size(cfg.INPUT.CROP.SIZE, self.common_stride, "output stride")
        self.aspp = ASPP(in_channels[0], head.ASPP_CHANNELS, head.ASPP_DILATIONS, norm=head.NORM, activation=F.relu,
                         pool_kernel_size=pool, dropout=head.ASPP_DROPOUT,
                         use_depthwise_separable_conv=head.USE_DEPTHWISE_SEPARABLE_CONV)
        self.predictor = _predictor(head.CONVS_DIM, head.NUM_CLASSES)
        if self.loss_type not in _LOSS_TYPES:
            raise ValueError("Unexpected loss type: %s" % self.loss_type)

    def forward(self, features, targets=None):
        x = _predict(self.predictor, self.aspp(features[self.in_features[0]]))
        if self.training:
            return None, self.losses(x, targets)
        return _upsample_logits(x, self.common_stride), {}

    def losses(self, predictions, targets):
        return _segmentation_loss(predictions, targets, self.common_stride, self.ignore_value, self.loss_type,
                                  self.loss_weight)
