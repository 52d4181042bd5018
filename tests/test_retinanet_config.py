"""The shipped RetinaNet configuration loads UNCHANGED through its _BASE_ chain — Base-RetinaNet.yaml writes the anchor
sizes behind a `!!python/object/apply:eval` tag, which the loader evaluates with an AST whitelist (build container only:
skipped where the reference tree is absent).  The flattened copy under tests/golden/configs/ (settings only, the 15
anchor sizes as literal numbers; what the GPU box can read) says the same on every MODEL key, anchor sizes to the last
bit, and builds RetinaNet with the reference's state-dict keys, shapes and initialisation."""
import math
import os

import pytest
import yaml

from conftest import GOLDEN

REF = "/root/reference/configs/COCO-Detection/retinanet_R_50_FPN_1x.yaml"
FLAT = os.path.join(GOLDEN, "configs", "retinanet_R_50_FPN_1x.yaml")
needs_reference = pytest.mark.skipif(not os.path.isfile(REF), reason="the reference tree exists in the build container only")
SIZES_TEXT = "[[x, x * 2**(1.0/3), x * 2**(2.0/3) ] for x in [32, 64, 128, 256, 512 ]]"


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
    from jtsm_amd.modeling import RetinaNet, RetinaNetHead
    from jtsm_amd.modeling.backbone import FPN, LastLevelP6P7

    assert type(model) is RetinaNet and type(model.head) is RetinaNetHead
    assert type(model.backbone) is FPN and type(model.backbone.top_block) is LastLevelP6P7
    assert model.backbone.size_divisibility == 128 and model.backbone.top_block.num_levels == 2
    assert list(model.backbone.output_shape()) == ["p3", "p4", "p5", "p6", "p7"]
    assert model.head_in_features == ["p3", "p4", "p5", "p6", "p7"] and model.num_classes == 80
    assert (model.focal_loss_alpha, model.focal_loss_gamma, model.smooth_l1_beta) == (0.25, 2.0, 0.0)
    assert (model.test_score_thresh, model.test_topk_candidates, model.test_nms_thresh) == (0.05, 1000, 0.5)
    assert model.max_detections_per_image == 100 and model.anchor_generator.num_cell_anchors == [9] * 5
    state = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    want = {"pixel_mean": (3, 1, 1), "pixel_std": (3, 1, 1),
            "head.cls_score.weight": (720, 256, 3, 3), "head.cls_score.bias": (720,),
            "head.bbox_pred.weight": (36, 256, 3, 3), "head.bbox_pred.bias": (36,),
            "backbone.top_block.p6.weight": (256, 2048, 3, 3), "backbone.top_block.p6.bias": (256,),
            "backbone.top_block.p7.weight": (256, 256, 3, 3), "backbone.top_block.p7.bias": (256,)}
    for tower in ("cls_subnet", "bbox_subnet"):
        for i in (0, 2, 4, 6):
            want["head.%s.%d.weight" % (tower, i)] = (256, 256, 3, 3)
            want["head.%s.%d.bias" % (tower, i)] = (256,)
    for level, c in ((3, 512), (4, 1024), (5, 2048)):
        want["backbone.fpn_lateral%d.weight" % level] = (256, c, 1, 1)
        want["backbone.fpn_lateral%d.bias" % level] = (256,)
        want["backbone.fpn_output%d.weight" % level] = (256, 256, 3, 3)
        want["backbone.fpn_output%d.bias" % level] = (256,)
    assert {k: v for k, v in state.items() if not k.startswith("backbone.bottom_up.")} == want
    assert "loss_normalizer" not in state and float(model.loss_normalizer) == 100.0
    head = model.head
    assert bool((head.cls_score.bias == -math.log(99)).all()) and not bool(head.bbox_pred.bias.any())
    assert abs(float(head.cls_subnet[0].weight.detach().std()) - 0.01) < 1e-3 and not bool(head.cls_subnet[0].bias.any())


@needs_reference
def test_reference_config_builds_unchanged():
    from jtsm_amd.modeling import build_model

    cfg = _cfg(REF)
    assert cfg.MODEL.META_ARCHITECTURE == "RetinaNet" and cfg.MODEL.RETINANET.SMOOTH_L1_LOSS_BETA == 0.0
    assert cfg.MODEL.ANCHOR_GENERATOR.SIZES == eval(SIZES_TEXT)          # the doubles Python's eval gives
    _check_built(build_model(cfg))


def test_flattened_copy_builds_the_same_model():
    from jtsm_amd.modeling import build_model

    text = open(FLAT).read()
    assert "!!" not in text and "eval" not in text                        # settings only
    cfg = _cfg(FLAT)
    sizes = cfg.MODEL.ANCHOR_GENERATOR.SIZES
    assert len(sizes) == 5 and all(len(s) == 3 for s in sizes)
    assert sizes == [[x, x * 2 ** (1.0 / 3), x * 2 ** (2.0 / 3)] for x in [32, 64, 128, 256, 512]]
    _check_built(build_model(cfg))


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

    r = get_cfg().MODEL.RETINANET
    assert (r.NUM_CLASSES, r.NUM_CONVS, r.PRIOR_PROB, r.NORM) == (80, 4, 0.01, "")
    assert r.IN_FEATURES == ["p3", "p4", "p5", "p6", "p7"] and r.IOU_THRESHOLDS == [0.4, 0.5] and r.IOU_LABELS == [0, -1, 1]
    assert (r.SCORE_THRESH_TEST, r.TOPK_CANDIDATES_TEST, r.NMS_THRESH_TEST) == (0.05, 1000, 0.5)
    assert tuple(r.BBOX_REG_WEIGHTS) == (1.0, 1.0, 1.0, 1.0) and r.BBOX_REG_LOSS_TYPE == "smooth_l1"
    assert (r.FOCAL_LOSS_GAMMA, r.FOCAL_LOSS_ALPHA, r.SMOOTH_L1_LOSS_BETA) == (2.0, 0.25, 0.1)


def test_eval_tag_gives_evals_doubles():
    from jtsm_amd.config.config import eval_arithmetic

    assert eval_arithmetic(SIZES_TEXT) == eval(SIZES_TEXT)
    assert eval_arithmetic("[-2 ** 0.5, (1 + 2) * 3 / 4 - 1, 1e-3]") == [-2 ** 0.5, (1 + 2) * 3 / 4 - 1, 1e-3]
    assert eval_arithmetic("(1, 2.5)") == (1, 2.5)


@pytest.mark.parametrize("text", [
    "__import__('os')", "().__class__", "abs(1)", "x + 1", "[y for x in [1, 2]]", "[x for x in range(3)]",
    "[x for x in [1, 2] if x]", "[[x for x in [1]] for y in [2]]", "'a' * 3", "[1, 2][0]", "lambda: 1", "1 if 2 else 3",
    "9 ** 9 ** 9", "True"])
def test_eval_tag_refuses_everything_else(text, tmp_path):
    from jtsm_amd.config import get_cfg
    from jtsm_amd.config.config import eval_arithmetic

    with pytest.raises(ValueError):
        eval_arithmetic(text)
    path = tmp_path / "bad.yaml"
    path.write_text("MODEL:\n  ANCHOR_GENERATOR:\n    SIZES: !!python/object/apply:eval [%s]\n" % yaml.safe_dump(text).strip())
    with pytest.raises(yaml.YAMLError):
        get_cfg().merge_from_file(str(path))


@pytest.mark.parametrize("tag", ["!!python/object/apply:os.system [\"true\"]", "!!python/name:os.system",
                                 "!!python/object/apply:eval [\"1\", \"2\"]", "!!python/object/apply:builtins.eval [\"1\"]"])
def test_other_python_tags_raise_as_before(tag, tmp_path):
    from jtsm_amd.config import get_cfg

    path = tmp_path / "bad.yaml"
    path.write_text("MODEL:\n  WEIGHTS: %s\n" % tag)
    with pytest.raises(yaml.YAMLError):
        get_cfg().merge_from_file(str(path))


def test_giou_is_refused():
    from jtsm_amd.modeling import build_model

    cfg = _cfg(FLAT)
    cfg.MODEL.RETINANET.BBOX_REG_LOSS_TYPE = "giou"
    with pytest.raises(NotImplementedError):
        build_model(cfg)
