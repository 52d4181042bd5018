"""Point head — surface of projects/PointRend/point_rend/point_head.py:15-157: POINT_HEAD_REGISTRY, StandardPointHead,
build_point_head (roi_mask_point_loss lives in layers/point_rend.py).

The MLP's kernel-1 Conv1d layers keep the reference's parameter names and shapes (`fc1.weight` is (256, 336, 1)) and run
as 1x1 contractions on the points-major row buffer the gather wrote: one row per point, fine-grained
features first, then the coarse prediction's C columns."""
import torch
import torch.nn.functional as F
from torch import nn

from ...layers.conv import linear_fused
from ...layers.shape_spec import ShapeSpec  # noqa: F401  (the reference's signature)
from ...layers.wrappers import _zero_padded_rows
from ...utils.registry import Registry

POINT_HEAD_REGISTRY = Registry("POINT_HEAD")


def contraction_rows(x, weight, bias, relu):
    """x (M, K) @ weight (O, K)^T + bias through the contraction kernels.  K and O are zero-padded to multiples of 8:
    narrower, the weight gradient falls to the kernel that adds its K slices with atomics (layers/wrappers.py) and two
    runs differ in their last bits.  Both paddings are sliced off again and receive no gradient.  At the shipped
    sizes (K = 336, 256; O = 256, 80) nothing is padded."""
    k, o = x.shape[1], weight.shape[0]
    if k % 8:
        x, weight = F.pad(x, (0, -k % 8)), F.pad(weight, (0, -k % 8))
    weight, bias = _zero_padded_rows(weight, bias, 8)
    y = linear_fused(x.contiguous(), weight.contiguous(), bias, relu, True)
    return y if y.shape[1] == o else y[:, :o]


@POINT_HEAD_REGISTRY.register()
class StandardPointHead(nn.Module):
    """point_head.py:99-149.  `forward_rows` is the path the mask head uses; `forward` keeps the reference's
    (R, C, P) signature on top of it."""

    def __init__(self, cfg, input_shape):
        super().__init__()
        p = cfg.MODEL.POINT_HEAD
        self.num_classes = p.NUM_CLASSES
        self.coarse_pred_each_layer = p.COARSE_PRED_EACH_LAYER
        fc_dim_in = input_shape.channels + self.num_classes
        self.fc_layers = []
        for k in range(p.NUM_FC):
            fc = nn.Conv1d(fc_dim_in, p.FC_DIM, kernel_size=1, stride=1, padding=0, bias=True)
            self.add_module("fc{}".format(k + 1), fc)
            self.fc_layers.append(fc)
            fc_dim_in = p.FC_DIM + (self.num_classes if self.coarse_pred_each_layer else 0)
        self.predictor = nn.Conv1d(fc_dim_in, 1 if p.CLS_AGNOSTIC_MASK else self.num_classes, kernel_size=1)
        for layer in self.fc_layers:          # c2_msra_fill
            nn.init.kaiming_normal_(layer.weight, mode="fan_out", nonlinearity="relu")
            nn.init.constant_(layer.bias, 0)
        nn.init.normal_(self.predictor.weight, std=0.001)
        nn.init.constant_(self.predictor.bias, 0)

    def forward_rows(self, rows, coarse_rows):
        """rows (M, fine + C): the gather's buffer; coarse_rows (M, C): its last C columns -> point logits (M, classes).
        With COARSE_PRED_EACH_LAYER the coarse columns are attached behind each layer's output by a concatenation (a
        layer that wrote into a wider buffer beside them would spare it; not built)."""
        x = rows
        for layer in self.fc_layers:
            x = contraction_rows(x, layer.weight.squeeze(-1), layer.bias, True)
            if self.coarse_pred_each_layer:
                x = torch.cat((x, coarse_rows), dim=1)
        return contraction_rows(x, self.predictor.weight.squeeze(-1), self.predictor.bias, False)

    def forward(self, fine_grained_features, coarse_features):
        r, c, p = coarse_features.shape
        x = torch.cat((fine_grained_features, coarse_features), dim=1).permute(0, 2, 1).reshape(r * p, -1)
        out = self.forward_rows(x, x[:, -c:])
        return out.view(r, p, -1).permute(0, 2, 1)


def build_point_head(cfg, input_channels):
    return POINT_HEAD_REGISTRY.get(cfg.MODEL.POINT_HEAD.NAME)(cfg, input_channels)
