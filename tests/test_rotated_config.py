"""Host-side pieces of the rotated-box path, on the CPU: RotatedAnchorGenerator against the expected tensor of the
reference's test_rrpn_anchor_generator, the Box2BoxTransformRotated round trip within the reference test's tolerances,
RotatedBoxes.normalize_angles / clip as the reference's test_normalize_angles / test_clip_area_0_degree state them, and
a config with RRPN, RotatedAnchorGenerator, RROIHeads, ROIAlignRotated and 5-tuple BBOX_REG_WEIGHTS through
build_model."""
import math
import os

import pytest
import torch

from conftest import ROOT


def rotated_cfg(device="cpu"):
    from jtsm_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "faster_rcnn_R_50_FPN_1x.yaml"))
    cfg.MODEL.DEVICE = device
    cfg.MODEL.PROPOSAL_GENERATOR.NAME = "RRPN"
    cfg.MODEL.ANCHOR_GENERATOR.NAME = "RotatedAnchorGenerator"
    cfg.MODEL.ANCHOR_GENERATOR.ANGLES = [[-60, 0, 60]]
    cfg.MODEL.RPN.BBOX_REG_WEIGHTS = (1.0, 1.0, 1.0, 1.0, 1.0)
    cfg.MODEL.ROI_HEADS.NAME = "RROIHeads"
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = 3
    cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE = "ROIAlignRotated"
    cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_WEIGHTS = (10.0, 10.0, 5.0, 5.0, 1.0)
    return cfg


def test_rotated_anchor_generator_matches_the_reference_tensor():
    from jtsm_amd.config import get_cfg
    from jtsm_amd.layers.shape_spec import ShapeSpec
    from jtsm_amd.modeling.anchor_generator import RotatedAnchorGenerator, build_anchor_generator
    from jtsm_amd.structures import RotatedBoxes

    cfg = get_cfg()
    cfg.MODEL.ANCHOR_GENERATOR.NAME = "RotatedAnchorGenerator"
    cfg.MODEL.ANCHOR_GENERATOR.SIZES = [[32, 64]]
    cfg.MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS = [[0.25, 1, 4]]
    cfg.MODEL.ANCHOR_GENERATOR.ANGLES = [0, 45]            # a single list
    gen = build_anchor_generator(cfg, [ShapeSpec(stride=4)])
    assert type(gen) is RotatedAnchorGenerator and gen.box_dim == 5 and gen.num_anchors == [12]
    anchors = gen([torch.rand(2, 96, 1, 2)])
    shapes = [(64.0, 16.0), (32.0, 32.0), (16.0, 64.0), (128.0, 32.0), (64.0, 64.0), (32.0, 128.0)]
    expected = torch.tensor([[x, 0.0, w, h, a] for x in (0.0, 4.0) for w, h in shapes for a in (0.0, 45.0)])
    assert isinstance(anchors[0], RotatedBoxes) and torch.allclose(anchors[0].tensor, expected)
    cfg.MODEL.ANCHOR_GENERATOR.ANGLES = [[0, 45]]          # a list of lists says the same
    assert torch.equal(build_anchor_generator(cfg, [ShapeSpec(stride=4)])([torch.rand(2, 96, 1, 2)])[0].tensor,
                       anchors[0].tensor)


def test_box2box_transform_rotated_round_trip():
    from jtsm_amd.modeling.box_regression import Box2BoxTransformRotated

    g = torch.Generator().manual_seed(3)
    t = Box2BoxTransformRotated(weights=(5, 5, 10, 10, 1))
    src = torch.rand(10, 5, generator=g)
    src[:, 2:4] += 1.0                                     # positive sides
    src[:, 4] = (src[:, 4] - 0.5) * 150
    dst = torch.rand(10, 5, generator=g)
    dst[:, 2:4] += 1.0
    dst[:, 4] = (dst[:, 4] - 0.5) * 150
    deltas = t.get_deltas(src, dst)
    assert deltas.shape == (10, 5)
    out = t.apply_deltas(deltas, src)
    assert torch.allclose(out[:, :4], dst[:, :4], atol=1e-5)
    assert torch.allclose((out[:, 4] - dst[:, 4] + 180.0) % 360.0 - 180.0, torch.zeros(10), atol=1e-4)
    far = dst.clone()
    far[:, 4] += 720.0                                     # the target's turn is taken modulo 360 ...
    assert torch.allclose(t.get_deltas(src, far), deltas, atol=1e-4)
    wide = t.apply_deltas(torch.cat([deltas, deltas], 1), src)     # ... and k classes decode side by side
    assert wide.shape == (10, 10) and torch.equal(wide[:, 5:], wide[:, :5]) and torch.equal(wide[:, :5], out)
    assert bool((out[:, 4] >= -180).all() and (out[:, 4] < 180).all())


def _random_boxes(g, n=100, turned=True):
    b = torch.zeros(n, 5)
    b[:, 0:2] = torch.rand(n, 2, generator=g) * 600 - 100
    b[:, 2:4] = torch.rand(n, 2, generator=g) * 500
    if turned:
        b[:, 4] = torch.rand(n, generator=g) * 3600 - 1800
    return b


def test_normalize_angles():
    from jtsm_amd.structures import RotatedBoxes

    g = torch.Generator().manual_seed(5)
    for _ in range(10):
        raw = _random_boxes(g)
        boxes = RotatedBoxes(raw.clone())
        boxes.normalize_angles()
        a = boxes.tensor[:, 4]
        assert bool((a >= -180).all() and (a < 180).all())
        assert torch.equal(boxes.tensor[:, :4], raw[:, :4])
        for f in (torch.cos, torch.sin):
            assert torch.allclose(f(raw[:, 4] * math.pi / 180), f(a * math.pi / 180), atol=1e-5)


def test_clip_area_0_degree():
    from jtsm_amd.structures import Boxes, RotatedBoxes

    g = torch.Generator().manual_seed(6)
    for _ in range(10):
        b5 = _random_boxes(g, turned=False)
        b4 = torch.stack([b5[:, 0] - b5[:, 2] / 2.0, b5[:, 1] - b5[:, 3] / 2.0, b5[:, 0] + b5[:, 2] / 2.0,
                          b5[:, 1] + b5[:, 3] / 2.0], 1)
        flat, turned = Boxes(b4), RotatedBoxes(b5)
        assert torch.allclose(flat.area(), turned.area(), atol=1e-1, rtol=1e-5)
        flat.clip((500, 600))
        turned.clip((500, 600))
        assert torch.allclose(flat.area(), turned.area(), atol=1e-1, rtol=1e-5)


def test_clip_leaves_turned_boxes_alone_and_scale_turns():
    from jtsm_amd.structures import RotatedBoxes

    g = torch.Generator().manual_seed(7)
    raw = _random_boxes(g)
    boxes = RotatedBoxes(raw.clone())
    before = boxes.area()
    boxes.clip((500, 600), clip_angle_threshold=30.0)
    shrunk = boxes.area() < before
    assert bool((boxes.area() <= before).all())
    assert bool((boxes.tensor[:, 4][shrunk].abs() <= 30.0).all())
    inside = RotatedBoxes(torch.tensor([[50.0, 50, 20, 10, 90], [5.0, 50, 20, 10, 0], [5.0, 50, 20, 4, 90]]))
    assert inside.inside_box((100, 100)).tolist() == [True, False, True]
    assert inside.nonempty(threshold=5).tolist() == [True, True, False]
    same = RotatedBoxes(torch.tensor([[10.0, 20, 30, 40, 30]]))
    same.scale(2.0, 2.0)
    assert torch.equal(same.tensor, torch.tensor([[20.0, 40, 60, 80, 30]]))
    quarter = RotatedBoxes(torch.tensor([[10.0, 20, 30, 40, 90], [10.0, 20, 30, 40, 0]]))
    quarter.scale(2.0, 3.0)      # at 90 degrees the width lies along y
    assert torch.allclose(quarter.tensor, torch.tensor([[20.0, 60, 90, 80, 90], [20.0, 60, 60, 120, 0]]), atol=1e-4)


def test_rotated_config_builds():
    from jtsm_amd.layers import ROIAlignRotated
    from jtsm_amd.modeling import RROIHeads, RRPN, RotatedAnchorGenerator, build_model
    from jtsm_amd.modeling.box_regression import Box2BoxTransformRotated
    from jtsm_amd.modeling.meta_arch.rcnn import GeneralizedRCNN
    from jtsm_amd.modeling.roi_heads import RotatedFastRCNNOutputLayers

    model = build_model(rotated_cfg())
    assert type(model) is GeneralizedRCNN
    rpn, heads = model.proposal_generator, model.roi_heads
    assert type(rpn) is RRPN and type(rpn.anchor_generator) is RotatedAnchorGenerator
    assert type(rpn.box2box_transform) is Box2BoxTransformRotated and len(rpn.box2box_transform.weights) == 5
    assert tuple(rpn.rpn_head.objectness_logits.weight.shape[:2]) == (9, 256)       # 1 size x 3 ratios x 3 angles
    assert tuple(rpn.rpn_head.anchor_deltas.weight.shape[:2]) == (45, 256)
    assert type(heads) is RROIHeads and all(type(p) is ROIAlignRotated for p in heads.box_pooler.level_poolers)
    pred = heads.box_predictor
    assert type(pred) is RotatedFastRCNNOutputLayers and type(pred.box2box_transform) is Box2BoxTransformRotated
    assert tuple(pred.bbox_pred.weight.shape) == (3 * 5, 1024) and tuple(pred.cls_score.weight.shape) == (4, 1024)
    keys = set(model.state_dict())
    assert {"proposal_generator.rpn_head.anchor_deltas.weight", "roi_heads.box_predictor.bbox_pred.weight",
            "roi_heads.box_head.fc1.weight"} <= keys


def test_rotated_heads_refuse_what_the_reference_refuses():
    from jtsm_amd.modeling import build_model

    cfg = rotated_cfg()
    cfg.MODEL.MASK_ON = True
    with pytest.raises(AssertionError):
        build_model(cfg)
    cfg = rotated_cfg()
    cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE = "ROIAlignV2"
    with pytest.raises(AssertionError):
        build_model(cfg)
    cfg = rotated_cfg()
    cfg.MODEL.RPN.BOUNDARY_THRESH = 0
    with pytest.raises(NotImplementedError):
        build_model(cfg)
    cfg = rotated_cfg()
    cfg.MODEL.ANCHOR_GENERATOR.NAME = "DefaultAnchorGenerator"
    with pytest.raises(ValueError):
        build_model(cfg)
