"""Build-container only (skipped where the reference tree is absent): the shipped ContextLocNet configuration loads
UNCHANGED through its _BASE_ chain and builds GeneralizedRCNNWSL / ContextLocNetROIHeads / a ROILoopPool pooler / the
DAN 25088 -> 4096 -> 4096 / cls and det 4096 -> 20; the flattened copy under tests/golden/configs/ (what the GPU tests
read) says the same as the reference-merged one on every MODEL / WSL key."""
import os

import pytest

from conftest import GOLDEN

REF = "/root/reference/projects/WSL/configs/PascalVOC-Detection/contextlocnet_WSR_18_DC5_1x.yaml"
FLAT = os.path.join(GOLDEN, "configs", "contextlocnet_WSR_18_DC5_1x.yaml")
pytestmark = pytest.mark.skipif(not os.path.isfile(REF), reason="the reference tree exists in the build container only")


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


def test_reference_config_builds_unchanged():
    from jtsm_amd.layers import ROILoopPool
    from jtsm_amd.modeling import build_model
    from jtsm_amd.modeling.meta_arch.rcnn_wsl import GeneralizedRCNNWSL
    from jtsm_amd.modeling.roi_heads.fast_rcnn_wsddn import WSDDNOutputLayers
    from jtsm_amd.modeling.roi_heads.roi_heads_contextlocnet import ContextLocNetROIHeads

    model = build_model(_cfg(REF))
    assert type(model) is GeneralizedRCNNWSL and type(model.roi_heads) is ContextLocNetROIHeads
    pools = list(model.roi_heads.box_pooler.level_poolers)
    assert len(pools) == 1 and type(pools[0]) is ROILoopPool and pools[0].spatial_scale == 0.125
    head = model.roi_heads.box_head
    assert [(fc.in_features, fc.out_features) for fc in head.fcs] == [(25088, 4096), (4096, 4096)]
    pred = model.roi_heads.box_predictor
    assert type(pred) is WSDDNOutputLayers and not pred.mean_loss
    assert tuple(pred.cls.weight.shape) == tuple(pred.det.weight.shape) == (20, 4096)
    assert not any(p.requires_grad for p in model.backbone.parameters())          # FREEZE_AT 5


def test_flattened_copy_agrees_with_the_merged_reference():
    ref, flat = _cfg(REF), _cfg(FLAT)
    for section in ("MODEL", "WSL"):
        a, b = _flat(ref[section]), _flat(flat[section])
        assert a.keys() == b.keys()
        diff = {k: (a[k], b[k]) for k in a if a[k] != b[k]}
        assert not diff, diff
