"""GPU suite (pytest -m gpu): ContextLocNet end to end — GeneralizedRCNNWSL + ContextLocNetROIHeads + WSDDNOutputLayers
on the shipped configuration (tests/golden/configs/contextlocnet_WSR_18_DC5_1x.yaml) against a CPU composition: the
oracle's ResNet-WS v2 dilated-C5 backbone (the one test_dc5_composite_matches_oracle uses), the ROILoopPool
restatement (tests/roi_loop_pool_ref.py), the DAN as F.linear + ReLU, cls(box) / det(frame) - det(context), the MIL
scores and image probabilities of oracle/model.py, BCE summed over classes / images (MEAN_LOSS False), and for
inference the oracle's per-class NMS."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import roi_loop_pool_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from jtsm_amd.config import add_wsl_config, get_cfg  # noqa: E402
from jtsm_amd.modeling import build_model  # noqa: E402

CFG = os.path.join(GOLDEN, "configs", "contextlocnet_WSR_18_DC5_1x.yaml")
HEAD = ["roi_heads.box_head.fc1", "roi_heads.box_head.fc2", "roi_heads.box_predictor.cls", "roi_heads.box_predictor.det"]


def _cfg(freeze_at=5):
    cfg = get_cfg()
    add_wsl_config(cfg)
    cfg.merge_from_file(CFG)
    cfg.MODEL.DEVICE = "cuda"
    # the oracle's backbone (resnet_wsl_v2.py); the shipped file names v1, whose pools sit one block later
    cfg.MODEL.BACKBONE.NAME = "build_wsl_resnet_v2_backbone"
    cfg.MODEL.BACKBONE.FREEZE_AT = freeze_at
    return cfg


def _params(seed=11):
    from oracle import model as OM
    p = OM.init_params_dc5(seed=seed, depth=18, nt=20, ns=2, dan_dims=(4096, 4096), input_gain=1.0 / 64)
    p = {k: v for k, v in p.items() if not k.startswith("roi_heads.") or k.startswith("roi_heads.box_head.")}
    g = torch.Generator().manual_seed(seed + 1)
    for n in ("cls", "det"):
        p["roi_heads.box_predictor.%s.weight" % n] = torch.randn(20, 4096, generator=g) * 0.01
        p["roi_heads.box_predictor.%s.bias" % n] = torch.randn(20, generator=g) * 0.01
    return p


def _batch(seed=77, R=300):
    from oracle import model as OM
    return OM.synthetic_batch(seed, B=2, size=256, R=R, sp_block=8, n_stuff=1, nt=20, ns=2)


def _model(p, freeze_at=5):
    model = build_model(_cfg(freeze_at))
    missing, unexpected = model.load_state_dict({k: v.detach() for k, v in p.items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    model.roi_heads.box_head.dropout_p = 0.0          # dropout masks frozen: none
    return model


def _cpu_logits(p, batch, res5_grad=False):
    """CPU composition of the forward up to (C, D); returns (C, D, counts, feature map)."""
    from oracle import model as OM
    x = OM.preprocess(p, batch["images"], 8)
    feat = OM.wsr_v2_dc5(p, x, 18)
    counts = [len(b) for b in batch["boxes"]]
    rois = torch.cat([torch.cat([torch.full((n, 1), float(i)), b], 1) for i, (n, b) in enumerate(zip(counts, batch["boxes"]))])
    _, arg = ref.forward(feat.detach().numpy(), rois.numpy(), 0.125, 7, 7)
    arg = torch.from_numpy(arg.astype(np.int64)).flatten(2)                       # (3R, C, 49)
    R = rois.shape[0]
    b = rois[:, 0].to(torch.int64).repeat(3)
    flat = feat.flatten(2)                                                          # (B, C, H*W)
    cidx = torch.arange(flat.shape[1])
    pooled = flat[b[:, None, None], cidx[None, :, None], arg.clamp(min=0)] * (arg >= 0).to(flat.dtype)
    scale = torch.cat([o + 1 for o in batch["objectness"]]).repeat(3)
    h = (pooled * scale.view(-1, 1, 1)).flatten(1)                                  # (c, h, w) column order
    for n in ("fc1", "fc2"):
        h = F.relu(F.linear(h, p["roi_heads.box_head.%s.weight" % n], p["roi_heads.box_head.%s.bias" % n]))
    cls = lambda t: F.linear(t, p["roi_heads.box_predictor.cls.weight"], p["roi_heads.box_predictor.cls.bias"])  # noqa
    det = lambda t: F.linear(t, p["roi_heads.box_predictor.det.weight"], p["roi_heads.box_predictor.det.bias"])  # noqa
    return cls(h[:R]), det(h[R:2 * R]) - det(h[2 * R:]), counts, feat


@pytest.fixture
def conv_math(request):
    from jtsm_amd.layers import conv as K
    old = K.MATH
    K.set_math(request.param)
    yield request.param
    K.set_math(old)


# (conv arithmetic, FREEZE_AT, loss bar, gradient bar): FREEZE_AT 4 trains res5, so the ROILoopPool backward runs
# inside autograd and res5's last convolution's gradient is compared too
# (gradient bar: L2 relative; fc1's bias gradient sums ~1800 gated rows, whose order differs: 1.03e-4 measured in f32)
STEP_CASES = [("f32", 5, 1e-4, 2e-4), ("bf16x3", 5, 1e-4, 1e-3), ("f32", 4, 1e-4, 2e-4)]


@pytest.mark.parametrize("conv_math,freeze_at,loss_bar,grad_bar", STEP_CASES, indirect=["conv_math"],
                         ids=["%s-freeze%d" % (m, f) for m, f, _, _ in STEP_CASES])
def test_training_step_matches_cpu_composition(cuda, conv_math, freeze_at, loss_bar, grad_bar):
    from model_util import to_batched_inputs
    from oracle import model as OM

    p = _params()
    batch = _batch()
    trained = [k for k in p if any(k.startswith(h + ".") for h in HEAD)]
    res5 = "backbone.res5.1.conv2.weight"
    if freeze_at == 4:
        trained.append(res5)
    for k in trained:
        p[k].requires_grad_(True)
    C, D, counts, _ = _cpu_logits(p, batch)
    probs = OM.mil_image_probs(OM.mil_scores(C, D, counts), counts)
    _, _, oh = OM.image_labels(batch["gt_classes"], batch["sem_seg"], 20, 2)
    loss0 = F.binary_cross_entropy(probs, oh[:, :20], reduction="sum") / len(counts)
    loss0.backward()

    model = _model(p, freeze_at)
    model.train()
    losses = model(to_batched_inputs(batch))
    assert set(losses) == {"loss_cls"}
    sum(losses.values()).backward()
    a, b = float(losses["loss_cls"].detach()), float(loss0.detach())
    assert abs(a - b) <= loss_bar * abs(b) + 1e-7, (a, b)
    got = dict(model.named_parameters())
    assert sorted(n for n, q in got.items() if q.requires_grad and n.startswith("roi_heads.")) == \
        sorted(k for k in trained if k.startswith("roi_heads."))
    worst = {}
    for n in trained:
        if n.endswith("box_predictor.det.bias"):
            continue   # exactly zero in exact arithmetic: det's bias cancels in det(frame) - det(context)
        g = got[n].grad
        assert g is not None, n
        if n.endswith("box_head.fc1.weight"):
            g = model.roi_heads.box_head._hwc_cols(g, False)
        g0 = p[n].grad
        d = g.detach().cpu().double() - g0.double()
        worst[n] = (d.norm() / (g0.double().norm() + 1e-12)).item()
    bar = {n: (5e-3 if n == res5 else grad_bar) for n in trained}
    bad = {n: v for n, v in worst.items() if v > bar[n]}
    assert not bad, bad


def test_frozen_backbone_runs_no_pooling_backward(cuda):
    """FREEZE_AT 5: the pooled rows carry no gradient, so the ROILoopPool backward never runs (counted through the
    library's call log) and no backbone parameter gets a gradient."""
    from model_util import to_batched_inputs
    from jtsm_amd import _lib as L

    model = _model(_params())
    model.train()
    inputs = to_batched_inputs(_batch(R=64))
    L.TIMING = []
    try:
        losses = model(inputs)
        names_fwd = [n for n, _, _ in L.TIMING]
        sum(losses.values()).backward()
        torch.cuda.synchronize()
        names = [n for n, _, _ in L.TIMING]
    finally:
        L.TIMING = None
    assert "jtsm_roi_loop_pool_forward_f32" in names_fwd
    assert "jtsm_roi_loop_pool_backward_f32" not in names
    assert all(q.grad is None for q in model.backbone.parameters())


def test_inference_matches_cpu_composition(cuda):
    from model_util import to_batched_inputs
    from oracle import inference as OI
    from oracle import model as OM

    p = _params()
    batch = _batch(R=200)
    with torch.no_grad():
        C, D, counts, _ = _cpu_logits(p, batch)
        scores0 = OM.mil_scores(C, D, counts)
    model = _model(p)
    model.roi_heads.box_predictor.test_score_thresh = 1e-5
    model.roi_heads.box_predictor.test_nms_thresh = 0.3
    model.eval()
    inputs = to_batched_inputs(batch)
    results, all_scores, all_boxes = model.inference(inputs, do_postprocess=False)
    out = model(inputs)
    assert len(out) == 2 and set(out[0]) == {"instances"}
    for i, (inst, sc, bx, img) in enumerate(zip(results, all_scores, all_boxes, batch["images"])):
        # the scores agree with the CPU composition's; near-equal scores may trade places at the top-100 cut, so the
        # selection is checked on the product's own scores and boxes
        s0 = scores0.split(counts)[i]
        assert torch.allclose(sc[0][:, :20].cpu(), s0, rtol=1e-4, atol=1e-5 * float(s0.max()))
        # the product's own selection re-derived by the oracle NMS from the product's scores and boxes
        want = OI.fast_rcnn_inference_single_image(bx[0].cpu(), sc[0].cpu(), tuple(img.shape[-2:]), 1e-5, 0.3, 100)
        assert torch.equal(inst.pred_classes.cpu(), want["classes"]) and torch.equal(inst.pred_inds.cpu(), want["rows"])
