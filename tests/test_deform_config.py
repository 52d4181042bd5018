"""CPU suite: MODEL.RESNETS.DEFORM_ON_PER_STAGE / DEFORM_MODULATED / DEFORM_NUM_GROUPS through build_model — the Faster
R-CNN R50-FPN configuration with deformable res3..res5, as detectron2/modeling/backbone/resnet.py:589-640 builds it."""
import os

import pytest
import torch

from conftest import ROOT


def deform_cfg(device="cpu", modulated=False, groups=1, stages=(False, True, True, True)):
    from jtsm_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "faster_rcnn_R_50_FPN_1x.yaml"))
    cfg.MODEL.DEVICE = device
    cfg.MODEL.RESNETS.DEFORM_ON_PER_STAGE = list(stages)
    cfg.MODEL.RESNETS.DEFORM_MODULATED = modulated
    cfg.MODEL.RESNETS.DEFORM_NUM_GROUPS = groups
    return cfg


@pytest.mark.parametrize("modulated,groups,channels", [(False, 1, 18), (True, 2, 54)])
def test_deformable_faster_rcnn_builds(modulated, groups, channels):
    from jtsm_amd.layers import DeformConv, ModulatedDeformConv
    from jtsm_amd.layers.wrappers import Conv2d
    from jtsm_amd.modeling import build_model
    from jtsm_amd.modeling.backbone.resnet import BottleneckBlock, DeformBottleneckBlock

    cfg = deform_cfg(modulated=modulated, groups=groups)
    model = build_model(cfg)
    bottom_up = model.backbone.bottom_up
    assert all(type(b) is BottleneckBlock for b in bottom_up.res2.children())
    assert not issubclass(DeformBottleneckBlock, BottleneckBlock)
    counts = {"res3": 4, "res4": 6, "res5": 3}
    for stage, n in counts.items():
        blocks = list(getattr(bottom_up, stage).children())
        assert len(blocks) == n and all(type(b) is DeformBottleneckBlock for b in blocks), stage
        for i, b in enumerate(blocks):
            assert b.deform_modulated == modulated
            assert type(b.conv2) is (ModulatedDeformConv if modulated else DeformConv)
            assert b.conv2.deformable_groups == groups and b.conv2.bias is None
            off = b.conv2_offset
            assert type(off) is Conv2d and off.norm is None and off.bias is not None
            assert off.out_channels == channels and off.kernel_size == (3, 3)
            in_3x3 = 2 if (i == 0 and not cfg.MODEL.RESNETS.STRIDE_IN_1X1) else 1  # the block's stride sits in one of them
            assert off.stride == (in_3x3, in_3x3) and b.conv1.stride == (2 // in_3x3 if i == 0 else 1,) * 2
            same = (lambda v: v if isinstance(v, tuple) else (v, v))
            assert same(b.conv2.stride) == off.stride and same(b.conv2.padding) == off.padding == (1, 1)
            assert float(off.weight.detach().abs().max()) == 0.0 and float(off.bias.detach().abs().max()) == 0.0
            assert float(b.conv2.weight.detach().abs().max()) > 0.0
            assert (b.shortcut is not None) == (i == 0)
    names = set(model.state_dict())
    for want in ("res3.0.conv1.weight", "res3.0.conv2_offset.weight", "res3.0.conv2_offset.bias", "res3.0.conv2.weight",
                 "res3.0.conv2.norm.weight", "res3.0.conv2.norm.running_var", "res3.0.conv3.weight",
                 "res3.0.shortcut.weight", "res5.2.conv2_offset.bias", "res5.2.conv2.norm.bias"):
        assert "backbone.bottom_up." + want in names, want
    assert "backbone.bottom_up.res3.0.conv2.bias" not in names
    assert "backbone.bottom_up.res2.0.conv2_offset.weight" not in names
    # FREEZE_AT = 2 leaves res3..res5 trainable
    assert bottom_up.res3[0].conv2_offset.weight.requires_grad and bottom_up.res3[0].conv2.weight.requires_grad
    assert "deformable_groups=%d" % groups in repr(bottom_up.res3[0].conv2)


def test_deformable_stage_by_stage():
    from jtsm_amd.modeling import build_model
    from jtsm_amd.modeling.backbone.resnet import BottleneckBlock, DeformBottleneckBlock

    bottom_up = build_model(deform_cfg(stages=(False, False, False, True))).backbone.bottom_up
    kinds = {s: {type(b) for b in getattr(bottom_up, s).children()} for s in ("res2", "res3", "res4", "res5")}
    assert kinds == {"res2": {BottleneckBlock}, "res3": {BottleneckBlock}, "res4": {BottleneckBlock},
                     "res5": {DeformBottleneckBlock}}


def test_deformable_r18_hits_the_reference_assertion():
    from jtsm_amd.modeling import build_model

    cfg = deform_cfg()
    cfg.MODEL.RESNETS.DEPTH = 18
    cfg.MODEL.RESNETS.RES2_OUT_CHANNELS = 64
    with pytest.raises(AssertionError, match="DEFORM_ON_PER_STAGE unsupported for R18/R34"):
        build_model(cfg)


def test_wsl_v2_builder_still_refuses_deformable_stages():
    from jtsm_amd.config import get_cfg
    from jtsm_amd.layers.shape_spec import ShapeSpec
    from jtsm_amd.modeling.backbone import resnet_wsl_v2

    builders = [getattr(resnet_wsl_v2, n) for n in dir(resnet_wsl_v2) if n.startswith("build_") and "backbone" in n]
    assert builders
    for build in builders:
        cfg = get_cfg()
        cfg.MODEL.RESNETS.DEFORM_ON_PER_STAGE = [False, False, False, True]
        with pytest.raises(NotImplementedError, match="deformable"):
            build(cfg, ShapeSpec(channels=3))


def test_deformable_ops_refuse_cpu_tensors():
    from jtsm_amd.layers import DeformConv

    with pytest.raises(RuntimeError, match="HIP device"):
        DeformConv(8, 8, 3, padding=1)(torch.zeros(1, 8, 5, 5), torch.zeros(1, 18, 5, 5))
