"""The shipped Keypoint R-CNN configuration loads UNCHANGED through its _BASE_ chain (build container only: skipped
where the reference tree is absent) and builds GeneralizedRCNN / RPN / StandardROIHeads with a keypoint pooler at
14 x 14 and KRCNNConvDeconvUpsampleHead (8 x 512, 17 keypoints).  The flattened copy under tests/golden/configs/ (what
the GPU box can read) builds the same model and says the same as the reference-merged one on every MODEL key.  The
head's state-dict keys and shapes are the reference's; the WSL and rotated heads still refuse KEYPOINT_ON."""
import os
import sys

import pytest

from conftest import GOLDEN, ROOT

REF = "/root/reference/configs/COCO-Keypoints/keypoint_rcnn_R_50_FPN_1x.yaml"
FLAT = os.path.join(GOLDEN, "configs", "keypoint_rcnn_R_50_FPN_1x.yaml")
needs_reference = pytest.mark.skipif(not os.path.isfile(REF), reason="the reference tree exists in the build container only")


def _cfg(path):
    from jtsm_amd.config import get_cfg
    cfg = get_cfg()
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
    from jtsm_amd.layers import ROIAlign
    from jtsm_amd.modeling.meta_arch.rcnn import GeneralizedRCNN
    from jtsm_amd.modeling.roi_heads import KRCNNConvDeconvUpsampleHead, StandardROIHeads

    assert type(model) is GeneralizedRCNN and type(model.roi_heads) is StandardROIHeads
    heads = model.roi_heads
    assert heads.keypoint_on and not heads.mask_on and heads.num_classes == 1
    assert tuple(heads.keypoint_pooler.output_size) == (14, 14) and len(heads.keypoint_pooler.level_poolers) == 4
    assert all(type(p) is ROIAlign and p.aligned for p in heads.keypoint_pooler.level_poolers)
    head = heads.keypoint_head
    assert type(head) is KRCNNConvDeconvUpsampleHead and head.num_keypoints == 17
    assert head.loss_normalizer == "visible" and head.loss_weight == 1.0 and head.up_scale == 2.0
    shapes = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    want = {"score_lowres.weight": (512, 17, 4, 4), "score_lowres.bias": (17,)}
    for i in range(1, 9):
        want["conv_fcn%d.weight" % i] = (512, 256 if i == 1 else 512, 3, 3)
        want["conv_fcn%d.bias" % i] = (512,)
    assert shapes == want
    assert not any(float(v.abs().max()) for k, v in head.state_dict().items() if k.endswith("bias"))
    assert all(float(v.std()) > 0 for k, v in head.state_dict().items() if k.endswith("weight"))
    assert {"roi_heads.keypoint_head.conv_fcn1.weight", "roi_heads.keypoint_head.score_lowres.weight"} <= set(model.state_dict())


@needs_reference
def test_reference_config_builds_unchanged():
    from jtsm_amd.modeling import build_model

    cfg = _cfg(REF)
    assert cfg.MODEL.KEYPOINT_ON is True and cfg.MODEL.RPN.POST_NMS_TOPK_TRAIN == 1500
    _check_built(build_model(cfg))


def test_flattened_copy_builds_the_same_model():
    from jtsm_amd.modeling import build_model

    _check_built(build_model(_cfg(FLAT)))


@needs_reference
def test_flattened_copy_agrees_with_the_merged_reference():
    ref, flat = _cfg(REF), _cfg(FLAT)
    for section in ("MODEL", "INPUT", "TEST"):
        a, b = _flat(ref[section]), _flat(flat[section])
        assert a.keys() == b.keys()
        diff = {k: (a[k], b[k]) for k in a if a[k] != b[k]}
        assert not diff, diff
    assert (ref.SOLVER.MAX_ITER, ref.SOLVER.IMS_PER_BATCH) == (flat.SOLVER.MAX_ITER, flat.SOLVER.IMS_PER_BATCH) == (90000, 16)


def test_defaults_are_the_reference_values():
    from jtsm_amd.config import get_cfg

    k = get_cfg().MODEL.ROI_KEYPOINT_HEAD
    assert (k.NAME, k.POOLER_RESOLUTION, k.POOLER_SAMPLING_RATIO, k.POOLER_TYPE) == ("KRCNNConvDeconvUpsampleHead", 14, 0, "ROIAlignV2")
    assert tuple(k.CONV_DIMS) == (512,) * 8 and k.NUM_KEYPOINTS == 17 and k.MIN_KEYPOINTS_PER_IMAGE == 1
    assert k.NORMALIZE_LOSS_BY_VISIBLE_KEYPOINTS is True and k.LOSS_WEIGHT == 1.0
    assert get_cfg().TEST.KEYPOINT_OKS_SIGMAS == [] and get_cfg().MODEL.KEYPOINT_ON is False


def test_head_from_keywords_and_the_fixed_normalizer():
    from jtsm_amd.layers.shape_spec import ShapeSpec
    from jtsm_amd.modeling.roi_heads import ROI_KEYPOINT_HEAD_REGISTRY, KRCNNConvDeconvUpsampleHead, build_keypoint_head

    assert ROI_KEYPOINT_HEAD_REGISTRY.get("KRCNNConvDeconvUpsampleHead") is KRCNNConvDeconvUpsampleHead
    head = KRCNNConvDeconvUpsampleHead(ShapeSpec(channels=16, height=14, width=14), num_keypoints=5, conv_dims=(8, 8))
    assert sorted(head.state_dict()) == ["conv_fcn1.bias", "conv_fcn1.weight", "conv_fcn2.bias", "conv_fcn2.weight",
                                         "score_lowres.bias", "score_lowres.weight"]
    assert tuple(head.score_lowres.weight.shape) == (8, 5, 4, 4)
    cfg = _cfg(FLAT)
    cfg.MODEL.ROI_KEYPOINT_HEAD.NORMALIZE_LOSS_BY_VISIBLE_KEYPOINTS = False
    cfg.MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS = (8,)
    head = build_keypoint_head(cfg, ShapeSpec(channels=16, height=14, width=14))
    assert head.loss_normalizer == 17 * 512 * 0.25


def test_without_keypoints_the_keypoint_modules_stay_unloaded():
    """A model with KEYPOINT_ON false neither builds a keypoint head nor imports the keypoint modules (a fresh
    interpreter, since this process has them loaded)."""
    import subprocess

    code = ("import sys; sys.path.insert(0, %r); from jtsm_amd.config import get_cfg; "
            "from jtsm_amd.modeling import build_model; cfg = get_cfg(); "
            "cfg.merge_from_file(%r); cfg.MODEL.DEVICE = 'cpu'; m = build_model(cfg); "
            "assert not m.roi_heads.keypoint_on and not hasattr(m.roi_heads, 'keypoint_head'); "
            "bad = [k for k in sys.modules if k.endswith(('keypoint_head', 'layers.keypoint'))]; assert not bad, bad"
            % (ROOT, os.path.join(ROOT, "configs", "faster_rcnn_R_50_FPN_1x.yaml")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("flat", ["cmil_WSR_18_DC5_1x.yaml", "pcl_WSR_18_DC5_1x.yaml"])
def test_wsl_heads_still_refuse_keypoints(flat):
    from jtsm_amd.config import add_wsl_config, get_cfg
    from jtsm_amd.modeling import build_model

    cfg = get_cfg()
    add_wsl_config(cfg)
    cfg.merge_from_file(os.path.join(GOLDEN, "configs", flat))
    cfg.MODEL.DEVICE = "cpu"
    cfg.MODEL.KEYPOINT_ON = True
    with pytest.raises(NotImplementedError):
        build_model(cfg)


def test_rotated_heads_still_refuse_keypoints():
    from jtsm_amd.modeling import build_model
    from test_rotated_config import rotated_cfg

    cfg = rotated_cfg()
    cfg.MODEL.KEYPOINT_ON = True
    with pytest.raises(AssertionError):
        build_model(cfg)
