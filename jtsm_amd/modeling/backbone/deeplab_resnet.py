"""DeepLabStem and build_resnet_deeplab_backbone — class name, module names (stem.conv1 .. conv3) and config keys of
projects/DeepLab/deeplab/resnet.py:15-158: a three-convolution stem, res4 / res5 dilated instead of strided
(RES4_DILATION, RES5_DILATION) and a multi-grid of dilations inside res5 (RES5_MULTI_GRID), on the blocks of resnet.py.
With live norms (the DeepLab configs train with SyncBN from the first layer) every block runs conv by conv, each
convolution followed by the fused batch norm (+ shortcut) + ReLU pass; the fused bottleneck node needs frozen norms."""
import torch.nn.functional as F

from ...layers.batch_norm import get_norm
from ...layers.blocks import CNNBlockBase
from ...layers.elementwise import max_pool_3x3_s2
from ...layers.wrappers import Conv2d
from .build import BACKBONE_REGISTRY
from .resnet import BasicStem, BottleneckBlock, DeformBottleneckBlock, ResNet, _msra


class DeepLabStem(CNNBlockBase):
    """Three 3x3 convolutions (the first with stride 2), each + norm + ReLU, then max-pool 3x3 stride 2: stride 4."""

    def __init__(self, in_channels=3, out_channels=128, norm="BN"):
        super().__init__(in_channels, out_channels, 4)
        self.in_channels = in_channels
        half = out_channels // 2
        self.conv1 = Conv2d(in_channels, half, kernel_size=3, stride=2, padding=1, bias=False,
                            norm=get_norm(norm, half), activation=F.relu)
        self.conv2 = Conv2d(half, half, kernel_size=3, stride=1, padding=1, bias=False, norm=get_norm(norm, half),
                            activation=F.relu)
        self.conv3 = Conv2d(half, out_channels, kernel_size=3, stride=1, padding=1, bias=False,
                            norm=get_norm(norm, out_channels), activation=F.relu)
        for conv in (self.conv1, self.conv2, self.conv3):
            _msra(conv)

    def forward(self, x):
        return max_pool_3x3_s2(self.conv3(self.conv2(self.conv1(x))))


@BACKBONE_REGISTRY.register()
def build_resnet_deeplab_backbone(cfg, input_shape):
    r = cfg.MODEL.RESNETS
    norm = r.NORM
    if r.STEM_TYPE == "basic":
        stem = BasicStem(in_channels=input_shape.channels, out_channels=r.STEM_OUT_CHANNELS, norm=norm)
    elif r.STEM_TYPE == "deeplab":
        stem = DeepLabStem(in_channels=input_shape.channels, out_channels=r.STEM_OUT_CHANNELS, norm=norm)
    else:
        raise ValueError("Unknown stem type: {}".format(r.STEM_TYPE))
    res4_dilation, res5_dilation = r.RES4_DILATION, r.RES5_DILATION
    assert res4_dilation in {1, 2}, "res4_dilation cannot be {}.".format(res4_dilation)
    assert res5_dilation in {1, 2, 4}, "res5_dilation cannot be {}.".format(res5_dilation)
    if res4_dilation == 2:
        assert res5_dilation == 4          # always dilate res5 if res4 is dilated
    blocks_per_stage = {50: [3, 4, 6, 3], 101: [3, 4, 23, 3], 152: [3, 8, 36, 3]}[r.DEPTH]
    cin, cout, mid = r.STEM_OUT_CHANNELS, r.RES2_OUT_CHANNELS, r.NUM_GROUPS * r.WIDTH_PER_GROUP
    last = max({"res2": 2, "res3": 3, "res4": 4, "res5": 5}[f] for f in r.OUT_FEATURES)
    stages = []
    for idx, number in enumerate(range(2, last + 1)):
        dilation = {4: res4_dilation, 5: res5_dilation}.get(number, 1)
        first_stride = 1 if idx == 0 or dilation > 1 else 2
        n = blocks_per_stage[idx]
        kwargs = {"block_class": BottleneckBlock, "num_blocks": n, "stride_per_block": [first_stride] + [1] * (n - 1),
                  "in_channels": cin, "out_channels": cout, "norm": norm, "bottleneck_channels": mid,
                  "stride_in_1x1": r.STRIDE_IN_1X1, "num_groups": r.NUM_GROUPS}
        if r.DEFORM_ON_PER_STAGE[idx]:
            kwargs.update(block_class=DeformBottleneckBlock, deform_modulated=r.DEFORM_MODULATED,
                          deform_num_groups=r.DEFORM_NUM_GROUPS)
        if number == 5:
            kwargs["dilation_per_block"] = [dilation * mg for mg in r.RES5_MULTI_GRID]
        else:
            kwargs["dilation"] = dilation
        stages.append(ResNet.make_stage(**kwargs))
        cin, cout, mid = cout, cout * 2, mid * 2
    return ResNet(stem, stages, out_features=r.OUT_FEATURES).freeze(cfg.MODEL.BACKBONE.FREEZE_AT)
