"""GPU suite: PointRend end to end — GeneralizedRCNN + RPN + StandardROIHeads with the flattened shipped 1x config
(tests/golden/configs/pointrend_rcnn_R_50_FPN_1x_coco.yaml) shrunk to 3 classes, narrow heads and two 128 x 128
synthetic images whose instances carry elliptic bitmasks.

* a training step: finite loss_mask and loss_mask_point, a finite non-zero gradient on every mask_head parameter, and
  p2's gradient collected by the gradient fan;
* two seeded steps give the same bits;
* ROI_BOX_HEAD.TRAIN_ON_PRED_BOXES on and off both run and leave the box losses equal;
* inference: pred_masks (R, 1, 224, 224) in [0, 1];
* the default pooler type still builds the pooled mask head and trains."""
import os

import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FLAT = os.path.join(GOLDEN, "configs", "pointrend_rcnn_R_50_FPN_1x_coco.yaml")
C = 3


def pointrend_cfg(train_on_pred_boxes=True, pointrend=True):
    from jtsm_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(FLAT)
    cfg.MODEL.DEVICE = "cuda"
    cfg.MODEL.WEIGHTS = ""
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = C
    cfg.MODEL.POINT_HEAD.NUM_CLASSES = C
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = 0.0
    cfg.TEST.DETECTIONS_PER_IMAGE = 10
    cfg.MODEL.ROI_MASK_HEAD.FC_DIM = 64
    cfg.MODEL.POINT_HEAD.FC_DIM = 32
    cfg.MODEL.ROI_BOX_HEAD.TRAIN_ON_PRED_BOXES = train_on_pred_boxes
    if not pointrend:
        cfg.MODEL.ROI_MASK_HEAD.NAME = "MaskRCNNConvUpsampleHead"
        cfg.MODEL.ROI_MASK_HEAD.POOLER_TYPE = "ROIAlignV2"
        cfg.MODEL.ROI_MASK_HEAD.NUM_CONV = 1
        cfg.MODEL.ROI_MASK_HEAD.CONV_DIM = 32
    return cfg


def build(cfg):
    from jtsm_amd.modeling import build_model
    torch.manual_seed(0)
    m = build_model(cfg)
    with torch.no_grad():
        m.backbone.bottom_up.stem.conv1.weight.mul_(1.0 / 64)
        m.roi_heads.box_head.fc1.weight.mul_(0.02)
        head = m.roi_heads.mask_head
        if hasattr(head, "point_head"):       # predictions of order 1, so that uncertainties differ between points
            head.point_head.predictor.weight.mul_(100.0)
            head.coarse_head.prediction.weight.mul_(100.0)
    return m


def batch():
    from jtsm_amd.utils.synthetic import synthetic_inputs
    data = synthetic_inputs(77, batch=2, size=128, proposals=8, sp_block=32, n_things=3, num_things=3, device="cuda",
                            keypoints=1)
    out = []
    yy, xx = torch.meshgrid(torch.arange(128, device="cuda") + 0.5, torch.arange(128, device="cuda") + 0.5, indexing="ij")
    for d in data:
        inst = d["instances"]
        inst.remove("gt_keypoints")
        b = inst.gt_boxes.tensor
        cx, cy = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
        rx, ry = (b[:, 2] - b[:, 0]) / 2, (b[:, 3] - b[:, 1]) / 2
        inst.gt_masks = ((((xx[None] - cx[:, None, None]) / rx[:, None, None]) ** 2 +
                          ((yy[None] - cy[:, None, None]) / ry[:, None, None]) ** 2) <= 1).to(torch.uint8)
        out.append({"image": d["image"], "instances": inst})
    return out


@pytest.fixture(scope="module")
def model(cuda):
    return build(pointrend_cfg())


def step(model, seed=5):
    model.train()
    model.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    losses = model(batch())
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in losses.items()}


def test_training_step(model, cuda):
    from jtsm_amd.layers import grad_fan
    from jtsm_amd.modeling.roi_heads import PointRendMaskHead
    assert type(model.roi_heads.mask_head) is PointRendMaskHead and model.roi_heads.mask_pooler is None
    before = dict(grad_fan.STATS)
    losses = step(model)
    assert set(losses) == {"loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc", "loss_mask", "loss_mask_point"}
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    assert float(losses["loss_mask"]) > 0 and float(losses["loss_mask_point"]) > 0
    for name, p in model.roi_heads.mask_head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), name
    # p2 is read by the coarse grid and by the point gather: one fan node more than before, and the FPN's p2
    # convolution has its gradient
    assert grad_fan.STATS["nodes"] > before["nodes"]
    g = model.backbone.fpn_output2.weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and bool(g.any())
    stats = model.roi_heads.mask_head.accuracy_stats.cpu()
    assert 0 <= int(stats[0]) <= int(stats[1]) and int(stats[1]) % 196 == 0 and int(stats[1]) > 0


def test_two_seeded_steps_are_bit_identical(model, cuda):
    a = step(model)
    ga = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    b = step(model)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    for n, p in model.named_parameters():
        if p.grad is not None:
            assert torch.equal(ga[n], p.grad), n


def test_train_on_pred_boxes_on_and_off(model, cuda):
    on = step(model)
    off = step(build(pointrend_cfg(train_on_pred_boxes=False)))
    assert all(bool(torch.isfinite(v)) for v in off.values())
    for k in ("loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc"):
        assert torch.equal(on[k], off[k]), k
    assert not torch.equal(on["loss_mask"], off["loss_mask"])       # the mask branch saw other boxes


def test_inference(model, cuda):
    model.eval()
    results = model.inference(batch(), do_postprocess=False)
    assert len(results) == 2
    total = 0
    for inst in results:
        m = inst.pred_masks
        assert tuple(m.shape) == (len(inst), 1, 224, 224) and m.dtype == torch.float32
        assert float(m.min()) >= 0.0 and float(m.max()) <= 1.0 and bool(torch.isfinite(m).all())
        total += len(inst)
    assert total > 0


def test_default_pooler_type_still_builds_and_trains(cuda):
    from jtsm_amd.modeling.roi_heads import MaskRCNNConvUpsampleHead
    m = build(pointrend_cfg(train_on_pred_boxes=False, pointrend=False))
    assert type(m.roi_heads.mask_head) is MaskRCNNConvUpsampleHead and m.roi_heads.mask_pooler is not None
    losses = step(m)
    assert "loss_mask_point" not in losses and bool(torch.isfinite(losses["loss_mask"])) and float(losses["loss_mask"]) > 0
    assert all(p.grad is not None and bool(p.grad.any()) for p in m.roi_heads.mask_head.parameters())


def test_no_detections_return_the_coarse_logits(model, cuda):
    """No box passes the score threshold: the head returns the (0, C, 7, 7) coarse logits as the reference does, so
    pred_masks is empty at the coarse resolution."""
    model.eval()
    pred = model.roi_heads.box_predictor
    keep, pred.test_score_thresh = pred.test_score_thresh, 2.0
    try:
        results = model.inference(batch(), do_postprocess=False)
    finally:
        pred.test_score_thresh = keep
    assert len(results) == 2
    for inst in results:
        assert len(inst) == 0 and tuple(inst.pred_masks.shape) == (0, 1, 7, 7)


def test_step_without_foreground_rois(model, cuda):
    """Ground truth that no proposal overlaps and that is not appended: both mask losses are 0 with zero gradients."""
    model.train()
    model.zero_grad(set_to_none=True)
    heads = model.roi_heads
    keep, heads.proposal_append_gt = heads.proposal_append_gt, False
    data = batch()
    for d in data:
        from jtsm_amd.structures import Boxes
        d["instances"].gt_boxes = Boxes(torch.tensor([[0.0, 0.0, 0.5, 0.5]] * 3, device="cuda"))
    try:
        torch.manual_seed(5)
        losses = model(data)
    finally:
        heads.proposal_append_gt = keep
    assert float(losses["loss_mask"].detach()) == 0.0 and float(losses["loss_mask_point"].detach()) == 0.0
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    for name, p in heads.mask_head.named_parameters():
        assert p.grad is None or (bool(torch.isfinite(p.grad).all()) and not bool(p.grad.any())), name
