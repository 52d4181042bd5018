"""Build-container only (skipped where the reference tree is absent): the shipped PCL configuration loads UNCHANGED
through its _BASE_ chain and builds GeneralizedRCNNWSL / PCLROIHeads / a ROIPool pooler at 1/8 / the DAN
25088 -> 4096 -> 4096 / cls and det 4096 -> 20 / three refinement layers of 21 outputs; the flattened copy under
tests/golden/configs/ (what the GPU tests read) says the same as the reference-merged one on every MODEL / WSL key.
The head's refusals (mask, keypoint, regression variant) need no reference tree."""
import os

import pytest

from conftest import GOLDEN

REF = "/root/reference/projects/WSL/configs/PascalVOC-Detection/pcl_WSR_18_DC5_1x.yaml"
FLAT = os.path.join(GOLDEN, "configs", "pcl_WSR_18_DC5_1x.yaml")
needs_reference = pytest.mark.skipif(not os.path.isfile(REF), reason="the reference tree exists in the build container only")


def _cfg(path):
    from jtsm_amd.config import add_wsl_config, get_cfg
    cfg = get_cfg()
    add_wsl_config(cfg)
    cfg.merge_from_file(path)
    cfg.MODEL.DEVICE = "cpu"
    return cfg


def _flat(node, pre=""):
    out = {}
    for k, v in node.items():
        if hasattr(v, "items"):
            out.update(_flat(v, pre + k + "."))
        else:
            out[pre + k] = list(v) if isinstance(v, tuple) else v
    return out


def _check_built(model):
    from jtsm_amd.layers import ROIPool
    from jtsm_amd.modeling.meta_arch.rcnn_wsl import GeneralizedRCNNWSL
    from jtsm_amd.modeling.roi_heads import PCLROIHeads
    from jtsm_amd.modeling.roi_heads.fast_rcnn_oicr import OICROutputLayers
    from jtsm_amd.modeling.roi_heads.fast_rcnn_wsddn import WSDDNOutputLayers

    assert type(model) is GeneralizedRCNNWSL and type(model.roi_heads) is PCLROIHeads
    pools = list(model.roi_heads.box_pooler.level_poolers)
    assert len(pools) == 1 and type(pools[0]) is ROIPool and pools[0].spatial_scale == 0.125
    assert tuple(pools[0].output_size) == (7, 7)
    head = model.roi_heads.box_head
    assert [(fc.in_features, fc.out_features) for fc in head.fcs] == [(25088, 4096), (4096, 4096)]
    pred = model.roi_heads.box_predictor
    assert type(pred) is WSDDNOutputLayers and pred.mean_loss
    assert tuple(pred.cls.weight.shape) == tuple(pred.det.weight.shape) == (20, 4096)
    refinery = model.roi_heads.box_refinery
    assert len(refinery) == 3 and all(type(r) is OICROutputLayers and not r.has_reg for r in refinery)
    assert [tuple(r.cls_score.weight.shape) for r in refinery] == [(21, 4096)] * 3
    assert [r.refine_k for r in refinery] == [0, 1, 2]
    assert not any(p.requires_grad for p in model.backbone.parameters())          # FREEZE_AT 5


@needs_reference
def test_reference_config_builds_unchanged():
    from jtsm_amd.modeling import build_model

    _check_built(build_model(_cfg(REF)))


def test_flattened_copy_builds_the_same_model():
    from jtsm_amd.modeling import build_model

    _check_built(build_model(_cfg(FLAT)))


@needs_reference
def test_flattened_copy_agrees_with_the_merged_reference():
    ref, flat = _cfg(REF), _cfg(FLAT)
    for section in ("MODEL", "WSL"):
        a, b = _flat(ref[section]), _flat(flat[section])
        assert a.keys() == b.keys()
        diff = {k: (a[k], b[k]) for k in a if a[k] != b[k]}
        assert not diff, diff


@pytest.mark.parametrize("key,value", [("MODEL.MASK_ON", True), ("MODEL.KEYPOINT_ON", True),
                                       ("WSL.REFINE_REG", [False, False, True])])
def test_unimplemented_variants_are_refused(key, value):
    from jtsm_amd.modeling import build_model

    cfg = _cfg(FLAT)
    node = cfg
    parts = key.split(".")
    for p in parts[:-1]:
        node = node[p]
    node[parts[-1]] = value
    with pytest.raises(NotImplementedError):
        build_model(cfg)
