"""The shipped PointRend instance-segmentation configurations load UNCHANGED through their _BASE_ chains (build
container only: skipped where the reference tree is absent); the flattened copy of the 1x config under
tests/golden/configs/ says the same on every MODEL / INPUT / TEST key and builds PointRendMaskHead with the reference's
parameter names and shapes; a checkpoint with the old `mask_point_head.` / `mask_coarse_head.` prefixes loads through
PointRendROIHeads; and the new default keys leave the trees of the existing configs unchanged apart from themselves."""
import os

import pytest
import torch

from conftest import GOLDEN, ROOT

REF_DIR = "/root/reference/projects/PointRend/configs/InstanceSegmentation"
SHIPPED = ["pointrend_rcnn_R_50_FPN_1x_coco.yaml", "pointrend_rcnn_R_50_FPN_3x_coco.yaml",
           "pointrend_rcnn_R_101_FPN_3x_coco.yaml"]
FLAT = os.path.join(GOLDEN, "configs", "pointrend_rcnn_R_50_FPN_1x_coco.yaml")
needs_reference = pytest.mark.skipif(not os.path.isdir(REF_DIR), reason="the reference tree exists in the build container only")

MASK_HEAD_STATE = {
    "coarse_head.reduce_spatial_dim_conv.weight": (256, 256, 2, 2), "coarse_head.reduce_spatial_dim_conv.bias": (256,),
    "coarse_head.coarse_mask_fc1.weight": (1024, 12544), "coarse_head.coarse_mask_fc1.bias": (1024,),
    "coarse_head.coarse_mask_fc2.weight": (1024, 1024), "coarse_head.coarse_mask_fc2.bias": (1024,),
    "coarse_head.prediction.weight": (3920, 1024), "coarse_head.prediction.bias": (3920,),
    "point_head.fc1.weight": (256, 336, 1), "point_head.fc1.bias": (256,),
    "point_head.fc2.weight": (256, 336, 1), "point_head.fc2.bias": (256,),
    "point_head.fc3.weight": (256, 336, 1), "point_head.fc3.bias": (256,),
    "point_head.predictor.weight": (80, 336, 1), "point_head.predictor.bias": (80,),
}
NEW_KEYS = {"INPUT.COLOR_AUG_SSD", "INPUT.CROP.SINGLE_CATEGORY_MAX_AREA", "MODEL.ROI_MASK_HEAD.IN_FEATURES",
            "MODEL.ROI_MASK_HEAD.FC_DIM", "MODEL.ROI_MASK_HEAD.NUM_FC", "MODEL.ROI_MASK_HEAD.OUTPUT_SIDE_RESOLUTION",
            "MODEL.ROI_MASK_HEAD.POINT_HEAD_ON"}


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
    from jtsm_amd.modeling.roi_heads import CoarseMaskHead, PointRendMaskHead, StandardPointHead, StandardROIHeads

    heads = model.roi_heads
    assert isinstance(heads, StandardROIHeads) and heads.mask_pooler is None and heads.train_on_pred_boxes
    head = heads.mask_head
    assert type(head) is PointRendMaskHead and type(head.coarse_head) is CoarseMaskHead
    assert type(head.point_head) is StandardPointHead and head.point_head.coarse_pred_each_layer
    assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == MASK_HEAD_STATE
    assert head.mask_coarse_in_features == ["p2"] and head.mask_point_in_features == ["p2"]
    assert head._feature_scales == {"p2": 0.25, "p3": 0.125, "p4": 0.0625, "p5": 0.03125}
    assert (head.mask_point_train_num_points, head.mask_point_oversample_ratio,
            head.mask_point_importance_sample_ratio) == (196, 3, 0.75)
    assert (head.mask_point_subdivision_steps, head.mask_point_subdivision_num_points) == (5, 784)
    # initialisation as in the reference: normal(0.001) predictors, zero biases, MSRA / Xavier fills elsewhere
    assert abs(float(head.point_head.predictor.weight.detach().std()) - 0.001) < 2e-4
    assert abs(float(head.coarse_head.prediction.weight.std()) - 0.001) < 1e-4
    assert not any(bool(p.any()) for n, p in head.named_parameters() if n.endswith(".bias"))
    w = head.coarse_head.coarse_mask_fc2.weight
    assert abs(float(w.abs().max()) - (3.0 / 1024) ** 0.5) < 1e-3              # c2_xavier_fill: uniform(+-sqrt(3 / fan_in))
    assert abs(float(head.point_head.fc1.weight.std()) - (2.0 / 256) ** 0.5) < 5e-3     # c2_msra_fill: fan_out


@needs_reference
@pytest.mark.parametrize("name", SHIPPED)
def test_shipped_configs_load_unchanged(name):
    cfg = _cfg(os.path.join(REF_DIR, name))
    m = cfg.MODEL
    assert m.MASK_ON and m.ROI_MASK_HEAD.NAME == "PointRendMaskHead" and m.ROI_MASK_HEAD.POOLER_TYPE == ""
    assert m.ROI_BOX_HEAD.TRAIN_ON_PRED_BOXES and m.ROI_MASK_HEAD.POINT_HEAD_ON and cfg.INPUT.MASK_FORMAT == "bitmask"
    assert list(m.ROI_MASK_HEAD.IN_FEATURES) == ["p2"] and list(m.POINT_HEAD.IN_FEATURES) == ["p2"]
    assert m.RESNETS.DEPTH == (101 if "R_101" in name else 50)


@needs_reference
def test_reference_config_builds_unchanged():
    from jtsm_amd.modeling import build_model
    torch.manual_seed(0)
    _check_built(build_model(_cfg(os.path.join(REF_DIR, SHIPPED[0]))))


def test_flattened_copy_builds_the_same_model():
    from jtsm_amd.modeling import build_model
    text = open(FLAT).read()
    assert "!!" not in text and "_BASE_" not in text                       # settings only
    torch.manual_seed(0)
    _check_built(build_model(_cfg(FLAT)))


@needs_reference
def test_flattened_copy_agrees_with_the_merged_reference():
    ref, flat = _cfg(os.path.join(REF_DIR, SHIPPED[0])), _cfg(FLAT)
    for section in ("MODEL", "INPUT", "TEST"):
        a, b = _flat(ref[section]), _flat(flat[section])
        assert a.keys() == b.keys()
        diff = {k: (a[k], b[k]) for k in a if a[k] != b[k]}
        assert not diff, diff
    assert (ref.SOLVER.MAX_ITER, ref.SOLVER.IMS_PER_BATCH) == (flat.SOLVER.MAX_ITER, flat.SOLVER.IMS_PER_BATCH) == (90000, 16)


def test_old_checkpoint_prefixes_load_through_pointrend_roi_heads():
    from jtsm_amd.modeling import build_model
    cfg = _cfg(FLAT)
    cfg.MODEL.ROI_HEADS.NAME = "PointRendROIHeads"
    torch.manual_seed(0)
    model = build_model(cfg)
    from jtsm_amd.modeling.roi_heads import PointRendROIHeads
    assert type(model.roi_heads) is PointRendROIHeads
    state = model.state_dict()
    old = {}
    for k, v in state.items():
        k = k.replace("roi_heads.mask_head.point_head.", "roi_heads.mask_point_head.")
        k = k.replace("roi_heads.mask_head.coarse_head.", "roi_heads.mask_coarse_head.")
        old[k] = torch.full_like(v, 0.5) if "mask_" in k else v
    assert any(".mask_point_head." in k for k in old) and not any(".mask_head." in k for k in old)
    if hasattr(old, "_metadata"):
        del old._metadata
    model.load_state_dict(old, strict=True)
    assert all(bool((p == 0.5).all()) for p in model.roi_heads.mask_head.parameters())
    # the old config form: the coarse head named as the mask head
    cfg.MODEL.ROI_MASK_HEAD.NAME = "CoarseMaskHead"
    cfg.MODEL.ROI_MASK_HEAD.POOLER_TYPE = "ROIAlign"
    again = build_model(cfg)
    assert type(again.roi_heads.mask_head).__name__ == "PointRendMaskHead" and again.roi_heads.mask_pooler is None


def test_defaults_add_keys_and_change_none():
    """The PointRend keys are new; every other key of an existing config's tree keeps its value and the default
    pooler type and TRAIN_ON_PRED_BOXES leave StandardROIHeads as it was."""
    from jtsm_amd.config import get_cfg
    cfg = get_cfg()
    flat = _flat(cfg)
    assert NEW_KEYS <= set(flat) and {k for k in flat if k.startswith("MODEL.POINT_HEAD.")} == {
        "MODEL.POINT_HEAD." + k for k in ("NAME", "NUM_CLASSES", "IN_FEATURES", "TRAIN_NUM_POINTS", "OVERSAMPLE_RATIO",
                                          "IMPORTANCE_SAMPLE_RATIO", "SUBDIVISION_STEPS", "SUBDIVISION_NUM_POINTS", "FC_DIM",
                                          "NUM_FC", "CLS_AGNOSTIC_MASK", "COARSE_PRED_EACH_LAYER", "COARSE_SEM_SEG_HEAD_NAME")}
    p = cfg.MODEL.POINT_HEAD
    assert (p.NAME, p.NUM_CLASSES, p.TRAIN_NUM_POINTS, p.OVERSAMPLE_RATIO, p.IMPORTANCE_SAMPLE_RATIO) == (
        "StandardPointHead", 80, 196, 3, 0.75)
    assert (p.SUBDIVISION_STEPS, p.SUBDIVISION_NUM_POINTS, p.FC_DIM, p.NUM_FC) == (5, 784, 256, 3)
    assert p.COARSE_PRED_EACH_LAYER and not p.CLS_AGNOSTIC_MASK
    m = cfg.MODEL.ROI_MASK_HEAD
    assert (m.FC_DIM, m.NUM_FC, m.OUTPUT_SIDE_RESOLUTION, m.POINT_HEAD_ON, m.POOLER_TYPE) == (1024, 2, 7, False, "ROIAlignV2")
    assert cfg.MODEL.ROI_BOX_HEAD.TRAIN_ON_PRED_BOXES is False
    # an existing flattened config (recorded before these keys existed) still says what it said
    import yaml
    old = os.path.join(GOLDEN, "configs", "retinanet_R_50_FPN_1x.yaml")
    merged, text = _flat(_cfg(old)), _flat(yaml.safe_load(open(old)))
    for k, v in text.items():
        if k != "MODEL.DEVICE":
            assert merged[k] == (list(v) if isinstance(v, tuple) else v), k
    added = set(merged) - set(text)
    assert {k for k in added if "POINT_HEAD" in k or k in NEW_KEYS} == NEW_KEYS | {k for k in flat if k.startswith("MODEL.POINT_HEAD.")}
    cfg2 = _cfg(os.path.join(ROOT, "configs", "faster_rcnn_R_50_FPN_1x.yaml"))
    cfg2.MODEL.MASK_ON = True
    from jtsm_amd.modeling import build_model
    heads = build_model(cfg2).roi_heads
    assert heads.mask_pooler is not None and not heads.train_on_pred_boxes
