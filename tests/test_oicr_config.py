"""The shipped OICR configurations load UNCHANGED through their _BASE_ chain (build container only: skipped where the
reference tree is absent) and build GeneralizedRCNNWSL / OICRROIHeads / a ROIPool pooler at 1/8 / the DAN
25088 -> 4096 -> 4096 / cls and det 4096 -> 20: `reg_all_mist/oicr_WSR_18_DC5_1x` with four refinement layers that
regress, MIST mining and SMOOTH_L1_BETA 1, the base `oicr_WSR_18_DC5_1x` with three that do not.  The flattened copy
of the former under tests/golden/configs/ (what the GPU tests read) says the same as the reference-merged one on every
MODEL / WSL key.  The head's refusals need no reference tree."""
import os

import pytest

from conftest import GOLDEN

REF_DIR = "/root/reference/projects/WSL/configs/PascalVOC-Detection"
REF = os.path.join(REF_DIR, "reg_all_mist", "oicr_WSR_18_DC5_1x.yaml")
REF_BASE = os.path.join(REF_DIR, "oicr_WSR_18_DC5_1x.yaml")
FLAT = os.path.join(GOLDEN, "configs", "oicr_mist_WSR_18_DC5_1x.yaml")
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


def _check_built(model, branches=4, reg=True, mist=True, beta=1.0):
    from jtsm_amd.layers import ROIPool
    from jtsm_amd.modeling.meta_arch.rcnn_wsl import GeneralizedRCNNWSL
    from jtsm_amd.modeling.roi_heads import OICRROIHeads
    from jtsm_amd.modeling.roi_heads.fast_rcnn_oicr import OICROutputLayers
    from jtsm_amd.modeling.roi_heads.fast_rcnn_wsddn import WSDDNOutputLayers

    assert type(model) is GeneralizedRCNNWSL and type(model.roi_heads) is OICRROIHeads
    assert model.roi_heads.refine_mist is mist
    pools = list(model.roi_heads.box_pooler.level_poolers)
    assert len(pools) == 1 and type(pools[0]) is ROIPool and pools[0].spatial_scale == 0.125
    assert tuple(pools[0].output_size) == (7, 7)
    head = model.roi_heads.box_head
    assert [(fc.in_features, fc.out_features) for fc in head.fcs] == [(25088, 4096), (4096, 4096)]
    pred = model.roi_heads.box_predictor
    assert type(pred) is WSDDNOutputLayers and pred.mean_loss
    assert tuple(pred.cls.weight.shape) == tuple(pred.det.weight.shape) == (20, 4096)
    refinery = model.roi_heads.box_refinery
    assert len(refinery) == branches and all(type(r) is OICROutputLayers and r.has_reg is reg for r in refinery)
    assert [tuple(r.cls_score.weight.shape) for r in refinery] == [(21, 4096)] * branches
    assert [tuple(r.bbox_pred.weight.shape) for r in refinery] == [(80, 4096)] * branches
    assert [r.refine_k for r in refinery] == list(range(branches))
    assert all(r.smooth_l1_beta == beta for r in refinery)
    assert not any(p.requires_grad for p in model.backbone.parameters())          # FREEZE_AT 5


@needs_reference
def test_reference_config_builds_unchanged():
    from jtsm_amd.modeling import build_model

    _check_built(build_model(_cfg(REF)))


@needs_reference
def test_reference_base_config_builds_unchanged():
    from jtsm_amd.modeling import build_model

    _check_built(build_model(_cfg(REF_BASE)), branches=3, reg=False, mist=False, beta=0.0)


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


def test_sampling_keys_carry_the_reference_defaults():
    s = _cfg(FLAT).WSL.SAMPLING
    assert s.SAMPLING_ON is False and [list(x) for x in s.IOU_THRESHOLDS] == [[0.5]] * 4
    assert [list(x) for x in s.IOU_LABELS] == [[0, 1]] * 4
    assert list(s.BATCH_SIZE_PER_IMAGE) == [4096] * 4 and list(s.POSITIVE_FRACTION) == [1.0] * 4


@pytest.mark.parametrize("beta", [0.0, 0.11])
def test_smooth_l1_beta_reaches_the_refinery(beta):
    from jtsm_amd.modeling import build_model

    cfg = _cfg(FLAT)
    cfg.MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA = beta
    assert all(r.smooth_l1_beta == beta for r in build_model(cfg).roi_heads.box_refinery)


def test_the_head_is_registered():
    from jtsm_amd.modeling.roi_heads import ROI_HEADS_REGISTRY, OICRROIHeads

    assert ROI_HEADS_REGISTRY.get("OICRROIHeads") is OICRROIHeads
