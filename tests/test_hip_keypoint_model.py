"""GPU suite: Keypoint R-CNN end to end — GeneralizedRCNN + RPN + StandardROIHeads with MODEL.KEYPOINT_ON on the R-50
FPN backbone the other detector tests build (the smallest the shared configs offer), two 128 x 128 synthetic images
with keypoints (jtsm_amd.utils.synthetic, keypoints=5), CONV_DIMS (32, 32), NUM_KEYPOINTS 5.

* a training step: loss_keypoint present and finite, a finite non-zero gradient on every keypoint-head parameter;
* the head alone against the same head written with torch ops in fp64 on the host, on the same pooled features:
  loss and parameter gradients within 1e-4 (f32 contractions) / 1e-3 (bf16x3);
* a batch whose keypoints are all v = 0: the step runs, the loss is 0, the head's gradients are zero and not NaN;
* inference: pred_keypoints (Ri, 5, 3) inside their boxes with scores in (0, 1], pred_keypoint_heatmaps
  (Ri, 5, 56, 56), and detector_postprocess to twice the size scales the points by exactly 2;
* with KEYPOINT_ON false, losses and detections for a fixed seed are bit-identical to those of a fresh interpreter
  that never imported the keypoint modules."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

pytestmark = pytest.mark.gpu

K, SIDE = 5, 56


def keypoint_cfg(keypoints=True):
    from jtsm_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "faster_rcnn_R_50_FPN_1x.yaml"))
    cfg.MODEL.DEVICE = "cuda"
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = 3
    cfg.TEST.DETECTIONS_PER_IMAGE = 20
    if keypoints:
        cfg.MODEL.KEYPOINT_ON = True
        cfg.MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS = (32, 32)
        cfg.MODEL.ROI_KEYPOINT_HEAD.NUM_KEYPOINTS = K
    return cfg


def build(cfg):
    from jtsm_amd.modeling import build_model
    torch.manual_seed(0)
    m = build_model(cfg)
    with torch.no_grad():
        m.backbone.bottom_up.stem.conv1.weight.mul_(1.0 / 64)
        m.roi_heads.box_head.fc1.weight.mul_(0.02)
        if cfg.MODEL.KEYPOINT_ON:
            # logits of order 1, as a trained head's: at initialisation they span hundreds, and where the bicubic
            # overshoot of such a map passes its largest pool-resolution value by more than log(S * S) the score
            # 1 / sum exp(map - max) exceeds 1 (in the reference too)
            m.roi_heads.keypoint_head.score_lowres.weight.mul_(0.01)
    return m


def batch(keypoints=K):
    from jtsm_amd.utils.synthetic import synthetic_inputs
    data = synthetic_inputs(77, batch=2, size=128, proposals=8, sp_block=32, n_things=3, num_things=3, device="cuda",
                            keypoints=K)
    out = [{"image": d["image"], "instances": d["instances"]} for d in data]
    if keypoints is None:
        for d in out:
            d["instances"].remove("gt_keypoints")
    return out


@pytest.fixture(scope="module")
def model(cuda):
    return build(keypoint_cfg())


def test_synthetic_keypoints(cuda):
    from jtsm_amd.utils.synthetic import synthetic_inputs
    plain = synthetic_inputs(77, batch=2, size=128, proposals=8, sp_block=32, n_things=3, num_things=3)
    with_kp = synthetic_inputs(77, batch=2, size=128, proposals=8, sp_block=32, n_things=3, num_things=3, keypoints=K)
    for a, b in zip(plain, with_kp):
        assert torch.equal(a["image"], b["image"]) and torch.equal(a["proposals"].proposal_boxes.tensor,
                                                                   b["proposals"].proposal_boxes.tensor)
        assert not a["instances"].has("gt_keypoints")
        kp, box = b["instances"].gt_keypoints.tensor, b["instances"].gt_boxes.tensor
        assert tuple(kp.shape) == (3, K, 3)
        lab = kp[:, :, 2] > 0
        assert lab.any() and (~lab).any() and not kp[~lab].any()
        inside = (kp[:, :, 0] >= box[:, None, 0]) & (kp[:, :, 0] <= box[:, None, 2]) & \
                 (kp[:, :, 1] >= box[:, None, 1]) & (kp[:, :, 1] <= box[:, None, 3])
        assert inside[lab].all()
        assert ((kp[:, :, 0] == box[:, None, 2]) & lab).any() and ((kp[:, :, 1] == box[:, None, 3]) & lab).any()


def test_training_step(model, cuda):
    model.train()
    model.zero_grad(set_to_none=True)
    losses = model(batch())
    assert set(losses) == {"loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc", "loss_keypoint"}
    assert all(bool(torch.isfinite(v)) for v in losses.values()) and float(losses["loss_keypoint"].detach()) > 0
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    for name, p in model.roi_heads.keypoint_head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), name


def test_step_without_a_labelled_keypoint(model, cuda):
    model.train()
    model.zero_grad(set_to_none=True)
    data = batch()
    for d in data:
        d["instances"].gt_keypoints.tensor.zero_()
    losses = model(data)
    assert float(losses["loss_keypoint"].detach()) == 0.0
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    for name, p in model.roi_heads.keypoint_head.named_parameters():
        assert p.grad is None or (bool(torch.isfinite(p.grad).all()) and not p.grad.any()), name
    assert model.roi_heads.box_head.fc1.weight.grad.any()


@pytest.fixture(params=["f32", "bf16x3"])
def conv_math(request):
    from jtsm_amd.layers import conv as CONV
    old = CONV.MATH
    CONV.set_math(request.param)
    CONV.planes_clear()
    yield request.param
    CONV.set_math(old)
    CONV.planes_clear()


def test_head_against_torch_ops(cuda, conv_math):
    from jtsm_amd.layers.shape_spec import ShapeSpec
    from jtsm_amd.modeling.roi_heads.keypoint_head import KRCNNConvDeconvUpsampleHead
    from jtsm_amd.structures import Boxes, Instances, Keypoints

    torch.manual_seed(3)
    head = KRCNNConvDeconvUpsampleHead(ShapeSpec(channels=32, height=14, width=14), num_keypoints=K, conv_dims=(32, 32),
                                       loss_weight=1.0, loss_normalizer="visible").to(cuda)
    with torch.no_grad():
        for p in head.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    head.train()
    g = torch.Generator().manual_seed(4)
    counts = (4, 3)
    x = torch.randn(sum(counts), 32, 14, 14, generator=g).to(cuda).contiguous(memory_format=torch.channels_last)
    instances, offset = [], 0
    for n in counts:
        x1y1 = torch.rand(n, 2, generator=g) * 60
        wh = torch.rand(n, 2, generator=g) * 50 + 10
        boxes = torch.cat([x1y1, x1y1 + wh], 1)
        kp = torch.rand(n, K, 3, generator=g)
        kp[:, :, :2] = x1y1[:, None] + kp[:, :, :2] * wh[:, None] * 1.2       # a few fall outside
        kp[:, :, 2] = (kp[:, :, 2] * 3).floor()                               # v in {0, 1, 2}
        instances.append(Instances((128, 128), proposal_boxes=Boxes(boxes.to(cuda)), gt_keypoints=Keypoints(kp.to(cuda))))
    loss = head(x, instances)["loss_keypoint"]
    loss.backward()
    torch.cuda.synchronize()
    # the same head with torch ops, fp64 on the host
    tv = [i.gt_keypoints.to_heatmap(i.proposal_boxes.tensor, SIDE) for i in instances]
    targets = torch.cat([t.view(-1) for t, _ in tv]).cpu().long()
    valid = torch.cat([v.view(-1) for _, v in tv]).cpu().bool()
    assert 3 < int(valid.sum()) < valid.numel()
    ref = {n: p.detach().cpu().double().contiguous().requires_grad_() for n, p in head.named_parameters()}
    y = x.detach().cpu().double().contiguous()
    for i in (1, 2):
        y = F.relu(F.conv2d(y, ref["conv_fcn%d.weight" % i], ref["conv_fcn%d.bias" % i], padding=1))
    y = F.conv_transpose2d(y, ref["score_lowres.weight"], ref["score_lowres.bias"], stride=2, padding=1)
    y = F.interpolate(y, scale_factor=2.0, mode="bilinear", align_corners=False)
    assert tuple(y.shape) == (sum(counts), K, SIDE, SIDE)
    rows = valid.nonzero().squeeze(1)
    want = F.cross_entropy(y.view(-1, SIDE * SIDE)[rows], targets[rows], reduction="sum") / rows.numel()
    y.retain_grad()
    want.backward()
    # a gradient is judged against the largest |gradient| of its tensor — but score_lowres.bias: the soft-max over
    # space does not see a shift of a whole map, so that gradient is 0 up to rounding (1e-17 in fp64) and is judged
    # against the size of what it sums, the per-keypoint sum of |d loss / d logits|
    scale = {n: float(p.grad.abs().max()) for n, p in ref.items()}
    scale["score_lowres.bias"] = float(y.grad.abs().sum((0, 2, 3)).max())
    assert scale["score_lowres.bias"] > 0.1 and float(ref["score_lowres.bias"].grad.abs().max()) < 1e-12
    bar = 1e-4 if conv_math == "f32" else 1e-3
    got = float(loss.detach())
    print(conv_math, "loss", got, float(want.detach()))
    assert abs(got - float(want.detach())) <= bar * abs(float(want.detach()))
    logits = head.layers(x).detach().cpu().double()
    assert float((logits - y.detach()).abs().max()) <= bar * float(y.detach().abs().max())
    for n, p in head.named_parameters():
        err = float((p.grad.detach().cpu().double() - ref[n].grad).abs().max()) / scale[n]
        print(conv_math, n, err)
        assert err <= bar, (n, err)


def test_inference_and_postprocess(model, cuda):
    from jtsm_amd.modeling.postprocessing import detector_postprocess

    model.eval()
    results = model.inference(batch(None), do_postprocess=False)
    assert len(results) == 2 and sum(len(r) for r in results) > 0
    for r in results:
        n = len(r)
        kp, box = r.pred_keypoints, r.pred_boxes.tensor
        assert tuple(kp.shape) == (n, K, 3) and tuple(r.pred_keypoint_heatmaps.shape) == (n, K, SIDE, SIDE)
        w = (box[:, 2] - box[:, 0]).clamp(min=1)[:, None]
        h = (box[:, 3] - box[:, 1]).clamp(min=1)[:, None]
        assert bool(((kp[:, :, 0] >= box[:, None, 0]) & (kp[:, :, 0] <= box[:, None, 0] + w)).all())
        assert bool(((kp[:, :, 1] >= box[:, None, 1]) & (kp[:, :, 1] <= box[:, None, 1] + h)).all())
        assert bool(((kp[:, :, 2] > 0) & (kp[:, :, 2] <= 1)).all())
        scaled = r.pred_boxes.clone()
        scaled.scale(2.0, 2.0)
        scaled.clip((256, 256))
        keep = scaled.nonempty()
        before = kp.clone()
        post = detector_postprocess(r, 256, 256)
        assert torch.equal(r.pred_keypoints, before)                # the model's own result is left alone
        assert torch.equal(post.pred_keypoints[:, :, :2], before[keep][:, :, :2] * 2)
        assert torch.equal(post.pred_keypoints[:, :, 2], before[keep][:, :, 2])


def plain_rcnn_digest():
    """sha256 of a KEYPOINT_ON = false model's training losses and detections for a fixed seed."""
    m = build(keypoint_cfg(keypoints=False))
    data = batch(None)
    m.train()
    torch.manual_seed(1)
    losses = m(data)
    h = hashlib.sha256()
    for k in sorted(losses):
        h.update(k.encode() + losses[k].detach().cpu().numpy().tobytes())
    m.eval()
    for r in m.inference(data, do_postprocess=False):
        for t in (r.pred_boxes.tensor, r.scores, r.pred_classes):
            h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    assert not hasattr(m.roi_heads, "keypoint_head")
    return h.hexdigest()


def test_without_keypoints_nothing_changes(model, cuda):
    """`model` (built above) has loaded the keypoint modules into this process; a fresh interpreter has not."""
    assert "jtsm_amd.modeling.roi_heads.keypoint_head" in sys.modules
    mine = plain_rcnn_digest()
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_hip_keypoint_model as T; d = T.plain_rcnn_digest(); "
            "bad = [k for k in sys.modules if k.endswith(('keypoint_head', 'layers.keypoint'))]; assert not bad, bad; "
            "print('digest', d)" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    theirs = [l.split()[1] for l in r.stdout.splitlines() if l.startswith("digest ")]
    assert theirs == [mine]
