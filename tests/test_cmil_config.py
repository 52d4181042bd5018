"""The shipped C-MIL configuration loads UNCHANGED through its _BASE_ chain (build container only: skipped where the
reference tree is absent) and builds GeneralizedRCNNWSL / CMILROIHeads / a ROILoopPool pooler at 1/8 / the DAN
25088 -> 4096 -> 4096 / cls and det 4096 -> 20 with ROIMerge(max_epoch 40, size_epoch 1250) / three refinement layers
that do not regress / ROILabel(0.6, 0.4, 0.1, 32, 96, 1).  The flattened copy under tests/golden/configs/ (what the GPU
tests read) says the same as the reference-merged one on every MODEL / WSL key.  The head's refusals need no reference
tree."""
import os

import pytest

from conftest import GOLDEN

REF = "/root/reference/projects/WSL/configs/PascalVOC-Detection/cmil_WSR_18_DC5_1x.yaml"
FLAT = os.path.join(GOLDEN, "configs", "cmil_WSR_18_DC5_1x.yaml")
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
    from jtsm_amd.layers import ROILabel, ROILoopPool, ROIMerge
    from jtsm_amd.modeling.meta_arch.rcnn_wsl import GeneralizedRCNNWSL
    from jtsm_amd.modeling.roi_heads import CMILROIHeads
    from jtsm_amd.modeling.roi_heads.fast_rcnn_oicr import OICROutputLayers
    from jtsm_amd.modeling.roi_heads.fast_rcnn_wsddn import WSDDNOutputLayers

    assert type(model) is GeneralizedRCNNWSL and type(model.roi_heads) is CMILROIHeads
    heads = model.roi_heads
    pools = list(heads.box_pooler.level_poolers)
    assert len(pools) == 1 and type(pools[0]) is ROILoopPool and pools[0].spatial_scale == 0.125
    assert tuple(pools[0].output_size) == (7, 7) and heads.blocks == 3
    assert [(fc.in_features, fc.out_features) for fc in heads.box_head.fcs] == [(25088, 4096), (4096, 4096)]
    pred = heads.box_predictor
    assert type(pred) is WSDDNOutputLayers and pred.mean_loss and pred.cmil
    assert tuple(pred.cls.weight.shape) == tuple(pred.det.weight.shape) == (20, 4096)
    merge = pred.roi_merge
    assert type(merge) is ROIMerge and (merge.max_epoch, merge.size_epoch, merge.display) == (40, 1250, 320)
    assert merge.cur_iter == 0 and not list(merge.parameters())        # a host int, no Parameter P
    refinery = heads.box_refinery
    assert len(refinery) == 3 and all(type(r) is OICROutputLayers and r.has_reg is False for r in refinery)
    assert [tuple(r.cls_score.weight.shape) for r in refinery] == [(21, 4096)] * 3
    assert [r.refine_k for r in refinery] == [0, 1, 2]
    label = heads.roi_label
    assert type(label) is ROILabel
    assert (label.fg, label.bg_hi, label.bg_lo, label.num_pos, label.num_neg, label.top_k) == (0.6, 0.4, 0.1, 32, 96, 1)
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
    assert (ref.SOLVER.MAX_ITER, ref.SOLVER.IMS_PER_BATCH) == (flat.SOLVER.MAX_ITER, flat.SOLVER.IMS_PER_BATCH) == (50000, 4)


def _set(cfg, key, value):
    node = cfg
    parts = key.split(".")
    for p in parts[:-1]:
        node = node[p]
    node[parts[-1]] = value


@pytest.mark.parametrize("key", ["MODEL.MASK_ON", "MODEL.KEYPOINT_ON", "MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG",
                                 "MODEL.ROI_BOX_HEAD.TRAIN_ON_PRED_BOXES", "WSL.SAMPLING.SAMPLING_ON"])
def test_unimplemented_variants_are_refused(key):
    from jtsm_amd.modeling import build_model

    cfg = _cfg(FLAT)
    _set(cfg, key, True)
    with pytest.raises(NotImplementedError):
        build_model(cfg)


def test_the_head_is_registered():
    from jtsm_amd.modeling.roi_heads import ROI_HEADS_REGISTRY, CMILROIHeads

    assert ROI_HEADS_REGISTRY.get("CMILROIHeads") is CMILROIHeads


def test_without_cmil_no_merge_is_built():
    from jtsm_amd.modeling import build_model

    cfg = _cfg(FLAT)
    cfg.WSL.CMIL = False
    pred = build_model(cfg).roi_heads.box_predictor
    assert not pred.cmil and not hasattr(pred, "roi_merge")
    other = build_model(_cfg(os.path.join(GOLDEN, "configs", "contextlocnet_WSR_18_DC5_1x.yaml"))).roi_heads.box_predictor
    assert not other.cmil and not hasattr(other, "roi_merge")


def test_a_plain_pooler_builds_the_one_block_form():
    from jtsm_amd.modeling import build_model

    cfg = _cfg(FLAT)
    cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE = "ROIPool"
    assert build_model(cfg).roi_heads.blocks == 1
