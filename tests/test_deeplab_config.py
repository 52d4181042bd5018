"""CPU suite: the DeepLab configs load and build (no kernel runs: construction and state-dict names only).
tests/golden/configs/ holds the two shipped Cityscapes configs of projects/DeepLab with their _BASE_ chain merged
(settings only); where the reference tree is present the shipped files themselves are loaded, unchanged, through that
chain and must give the same configuration."""
import os

import pytest

from jtsm_amd.config import CfgNode, get_cfg
from jtsm_amd.modeling import build_model

HERE = os.path.dirname(os.path.abspath(__file__))
FLAT = os.path.join(HERE, "golden", "configs")
SHIPPED = "/root/reference/projects/DeepLab/configs/Cityscapes-SemanticSegmentation"
V3PLUS, V3 = "deeplab_v3_plus_R_103_os16_mg124_poly_90k_bs16", "deeplab_v3_R_103_os16_mg124_poly_90k_bs16"


def _cfg(path, *overrides):
    cfg = get_cfg()
    cfg.merge_from_file(path)
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(overrides))
    return cfg


@pytest.fixture(scope="module")
def models():
    return {name: build_model(_cfg(os.path.join(FLAT, name + ".yaml"))) for name in (V3PLUS, V3)}


def test_flattened_configs_build_with_the_checkpoint_names(models):
    sd = models[V3PLUS].state_dict()
    for key in ("backbone.stem.conv3.norm.running_var", "backbone.res5.2.conv2.norm.num_batches_tracked",
                "sem_seg_head.decoder.res5.project_conv.convs.0.norm.weight",
                "sem_seg_head.decoder.res5.project_conv.convs.4.1.bias",
                "sem_seg_head.decoder.res5.project_conv.project.weight", "sem_seg_head.decoder.res2.project_conv.weight",
                "sem_seg_head.decoder.res2.fuse_conv.1.norm.bias", "sem_seg_head.predictor.bias"):
        assert key in sd, key
    assert "sem_seg_head.aspp.convs.3.weight" in models[V3].state_dict()
    assert tuple(sd["sem_seg_head.predictor.weight"].shape) == (19, 256, 1, 1)
    assert tuple(sd["sem_seg_head.decoder.res2.fuse_conv.0.weight"].shape) == (256, 256 + 48, 3, 3)
    assert tuple(sd["backbone.stem.conv1.weight"].shape) == (64, 3, 3, 3)
    assert len(models[V3PLUS].backbone.res4) == 23                  # DEPTH 101 (the "R-103" of the file name: + the stem)


def test_res5_carries_the_multi_grid_dilations(models):
    for model in models.values():
        res5 = list(model.backbone.res5)
        assert [b.conv2.dilation for b in res5] == [(2, 2), (4, 4), (8, 8)]       # RES5_DILATION 2 x [1, 2, 4]
        assert [b.conv2.padding for b in res5] == [(2, 2), (4, 4), (8, 8)]
        assert [b.conv2.stride for b in res5] == [(1, 1)] * 3                      # dilated, not strided: stride 16
        assert model.backbone.output_shape()["res5"].stride == 16


def test_every_norm_is_live_and_sits_in_the_norm_weight_decay_group(models):
    import torch
    from jtsm_amd.layers.batch_norm import BatchNorm2d
    from jtsm_amd.solver.build import build_optimizer
    model = models[V3PLUS]
    norms = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(norms) > 100 and all(isinstance(m, BatchNorm2d) and m.sync for m in norms)
    assert all(p.requires_grad for p in model.parameters())         # FREEZE_AT 0
    cfg = _cfg(os.path.join(FLAT, V3PLUS + ".yaml"), "SOLVER.WEIGHT_DECAY_NORM", 0.25)
    opt = build_optimizer(cfg, model)
    norm_params = {id(p) for m in norms for p in m.parameters()}
    for group in opt.param_groups:
        for p in group["params"]:
            assert (group["weight_decay"] == 0.25) == (id(p) in norm_params)


@pytest.mark.parametrize("name", [V3PLUS, V3])
def test_shipped_configs_load_unchanged_and_agree_with_the_flattened_copies(name, models):
    if not os.path.isdir(SHIPPED):       # (the reference tree is in the build container only; elsewhere the committed
        return                           # copies are the pin, as for tests/golden/*.npz)
    shipped, flat = _cfg(os.path.join(SHIPPED, name + ".yaml")), _cfg(os.path.join(FLAT, name + ".yaml"))
    assert shipped.dump() == flat.dump()          # (dump writes tuples as lists: "(60000, 80000)" and [60000, 80000] agree)
    assert CfgNode(CfgNode.load_yaml_with_base(os.path.join(SHIPPED, name + ".yaml"))).dump() == \
        CfgNode(CfgNode.load_yaml_with_base(os.path.join(FLAT, name + ".yaml"))).dump()
    assert shipped.SOLVER.LR_SCHEDULER_NAME == "WarmupPolyLR" and shipped.INPUT.CROP.SIZE == [512, 1024]
    built = build_model(shipped)
    want = models[name].state_dict()
    assert {k: tuple(v.shape) for k, v in built.state_dict().items()} == {k: tuple(v.shape) for k, v in want.items()}


def test_defaults_add_keys_and_change_none():
    from jtsm_amd.config.defaults import _C, _DEEPLAB_DEFAULTS, add_wsl_config
    before = _C.clone()
    add_wsl_config(before)
    after = get_cfg()

    def walk(old, new, path=""):
        for k, v in old.items():
            assert k in new, path + k
            if isinstance(v, dict):
                walk(v, new[k], path + k + ".")
            else:
                assert new[k] == v and type(new[k]) is type(v), path + k
    walk(before, after)

    def added(node, new, old, path=""):
        for k, v in node.items():
            if isinstance(v, dict):
                added(v, new[k], old.get(k, {}), path + k + ".")
            else:
                assert new[k] == v, path + k
                assert k not in old or old[k] == v, path + k
    added(_DEEPLAB_DEFAULTS, after, before)
    # the reference's add_deeplab_config values
    assert after.MODEL.SEM_SEG_HEAD.LOSS_TYPE == "hard_pixel_mining" and after.MODEL.RESNETS.STEM_TYPE == "deeplab"
    assert after.MODEL.RESNETS.RES4_DILATION == 1 and after.MODEL.RESNETS.RES5_MULTI_GRID == [1, 2, 4]
    assert after.INPUT.CROP.ENABLED is False and after.SOLVER.LR_SCHEDULER_NAME == "WarmupMultiStepLR"


def test_depthwise_separable_conv_is_refused():
    with pytest.raises(NotImplementedError):
        build_model(_cfg(os.path.join(FLAT, V3PLUS + ".yaml"), "MODEL.SEM_SEG_HEAD.USE_DEPTHWISE_SEPARABLE_CONV", True))
    with pytest.raises(NotImplementedError):
        build_model(_cfg(os.path.join(FLAT, V3 + ".yaml"), "MODEL.SEM_SEG_HEAD.USE_DEPTHWISE_SEPARABLE_CONV", True))


def test_dilations_are_validated_as_the_reference_validates_them():
    path = os.path.join(FLAT, V3PLUS + ".yaml")
    with pytest.raises(AssertionError):
        build_model(_cfg(path, "MODEL.RESNETS.RES4_DILATION", 4))
    with pytest.raises(AssertionError):
        build_model(_cfg(path, "MODEL.RESNETS.RES5_DILATION", 3))
    with pytest.raises(AssertionError):
        build_model(_cfg(path, "MODEL.RESNETS.RES4_DILATION", 2, "MODEL.RESNETS.RES5_DILATION", 2))
    with pytest.raises(ValueError):
        build_model(_cfg(path, "MODEL.RESNETS.STEM_TYPE", "other"))
    model = build_model(_cfg(path, "MODEL.RESNETS.RES4_DILATION", 2, "MODEL.RESNETS.RES5_DILATION", 4,
                             "MODEL.RESNETS.DEPTH", 50, "MODEL.RESNETS.STEM_TYPE", "basic",
                             "MODEL.RESNETS.STEM_OUT_CHANNELS", 64))
    assert model.backbone.output_shape()["res5"].stride == 8
    assert [b.conv2.dilation[0] for b in model.backbone.res5] == [4, 8, 16]
