"""GPU suite (pytest -m gpu): PCL end to end — GeneralizedRCNNWSL + PCLROIHeads + WSDDNOutputLayers + three
OICROutputLayers branches on the shipped configuration (tests/golden/configs/pcl_WSR_18_DC5_1x.yaml) against a CPU
composition built as tests/test_hip_contextlocnet_model.py builds its own: the oracle's ResNet-WS v2 dilated-C5
backbone, the ROIPool restatement (tests/roi_pool_ref.py), the DAN as F.linear + ReLU, cls / det and the MIL scores of
oracle/model.py with BCE averaged over images x classes (MEAN_LOSS True), and per branch the PCL loss formula in torch
autograd with the DEVICE's cluster tables frozen in (which proposals are background, which cluster a proposal belongs
to, the centres' scores); pc_prob and everything downstream is recomputed on the CPU side.  Inference: the branches'
soft-max averaged, the background column moved behind the classes, the oracle's per-class NMS.
Cases and bars are that file's: loss 1e-4; gradients 2e-4 in f32 and 1e-3 in bf16x3 (L2 relative)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import roi_pool_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from jtsm_amd.config import add_wsl_config, get_cfg  # noqa: E402
from jtsm_amd.modeling import build_model  # noqa: E402

CFG = os.path.join(GOLDEN, "configs", "pcl_WSR_18_DC5_1x.yaml")
REFINE = ["roi_heads.box_refinery_%d.cls_score" % k for k in range(3)]
HEAD = ["roi_heads.box_head.fc1", "roi_heads.box_head.fc2", "roi_heads.box_predictor.cls",
        "roi_heads.box_predictor.det"] + REFINE


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
    for k in range(3):
        p[REFINE[k] + ".weight"] = torch.randn(21, 4096, generator=g) * 0.02
        p[REFINE[k] + ".bias"] = torch.randn(21, generator=g) * 0.01
    return p


def _batch(seed=77, R=300):
    from oracle import model as OM
    return OM.synthetic_batch(seed, B=2, size=256, R=R, sp_block=8, n_stuff=1, nt=20, ns=2)


def _model(p, freeze_at=5):
    model = build_model(_cfg(freeze_at))
    missing, unexpected = model.load_state_dict({k: v.detach() for k, v in p.items()}, strict=False)
    # (the branches' bbox_pred layers exist, as in the reference, and are unused without WSL.REFINE_REG)
    assert all(".bbox_pred." in k for k in missing) and not unexpected, (missing, unexpected)
    model.roi_heads.box_head.dropout_p = 0.0          # dropout masks frozen: none
    return model


def _cpu_logits(p, batch):
    """CPU composition of the forward up to the logits: (cls, det, [branch logits], counts)."""
    from oracle import model as OM
    x = OM.preprocess(p, batch["images"], 8)
    feat = OM.wsr_v2_dc5(p, x, 18)
    counts = [len(b) for b in batch["boxes"]]
    rois = torch.cat([torch.cat([torch.full((n, 1), float(i)), b], 1) for i, (n, b) in enumerate(zip(counts, batch["boxes"]))])
    _, arg = ref.forward(feat.detach().numpy(), rois.numpy(), 0.125, 7, 7)
    arg = torch.from_numpy(arg.astype(np.int64)).flatten(2)                       # (R, C, 49)
    b = rois[:, 0].to(torch.int64)
    flat = feat.flatten(2)                                                          # (B, C, H*W)
    cidx = torch.arange(flat.shape[1])
    pooled = flat[b[:, None, None], cidx[None, :, None], arg.clamp(min=0)] * (arg >= 0).to(flat.dtype)
    scale = torch.cat([o + 1 for o in batch["objectness"]])
    h = (pooled * scale.view(-1, 1, 1)).flatten(1)                                  # (c, h, w) column order
    for n in ("fc1", "fc2"):
        h = F.relu(F.linear(h, p["roi_heads.box_head.%s.weight" % n], p["roi_heads.box_head.%s.bias" % n]))
    lin = lambda name: F.linear(h, p[name + ".weight"], p[name + ".bias"])  # noqa: E731
    return (lin("roi_heads.box_predictor.cls"), lin("roi_heads.box_predictor.det"), [lin(n) for n in REFINE], counts)


def _cpu_pcl_loss(z, counts, t):
    """The PCL loss of one branch in torch autograd from logits z (R, 21) and the device's tables (numpy)."""
    p = torch.softmax(z, dim=1)
    total = 0.0
    lo = 0
    for i, n in enumerate(counts):
        pi = p[lo:lo + n]
        lab = torch.from_numpy(t["row_label"][lo:lo + n].astype(np.int64))
        asg = torch.from_numpy(t["row_assign"][lo:lo + n].astype(np.int64))
        w = torch.from_numpy(t["row_weight"][lo:lo + n])
        li = -(w[lab == 0] * torch.log(pi[lab == 0, 0].clamp_min(1e-6))).sum()
        for j in range(int(t["pc_num"][i])):
            m = asg == j
            cnt = int(m.sum())
            assert cnt == int(t["pc_int"][i, j, 1])
            if cnt:
                pc = pi[m, int(t["pc_int"][i, j, 0])].clamp(1e-9, 1 - 1e-9).mean()
                li = li - float(t["pc_flt"][i, j, 0]) * cnt * torch.log(pc.clamp_min(1e-6))
        total = total + li / n
        lo += n
    return total / len(counts)


@pytest.fixture
def conv_math(request):
    from jtsm_amd.layers import conv as K
    old = K.MATH
    K.set_math(request.param)
    yield request.param
    K.set_math(old)


# (conv arithmetic, FREEZE_AT, loss bar, gradient bar): FREEZE_AT 4 trains res5, so the ROIPool backward runs inside
# autograd and res5's last convolution's gradient is compared too
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

    model = _model(p, freeze_at)
    model.train()
    losses = model(to_batched_inputs(batch))
    assert set(losses) == {"loss_cls", "loss_cls_r0", "loss_cls_r1", "loss_cls_r2"}
    sum(losses.values()).backward()
    tables = [{k: v.cpu().numpy() for k, v in t.items()} for t in model.roi_heads.aux["pcl_tables"]]
    assert all(int(t["pc_num"].min()) >= 1 and (t["row_label"] > 0).any() for t in tables)   # clusters with members

    for k in trained:
        p[k].requires_grad_(True)
    C, D, Z, counts = _cpu_logits(p, batch)
    probs = OM.mil_image_probs(OM.mil_scores(C, D, counts), counts)
    _, _, oh = OM.image_labels(batch["gt_classes"], batch["sem_seg"], 20, 2)
    want = {"loss_cls": F.binary_cross_entropy(probs, oh[:, :20], reduction="mean")}
    for k in range(3):
        want["loss_cls_r%d" % k] = _cpu_pcl_loss(Z[k], counts, tables[k])
    sum(want.values()).backward()
    for k, v in want.items():
        a, b = float(losses[k].detach()), float(v.detach())
        print("%s: device %.8g cpu %.8g rel %.3g" % (k, a, b, abs(a - b) / abs(b)))
        assert abs(a - b) <= loss_bar * abs(b) + 1e-7, (k, a, b)
    got = dict(model.named_parameters())
    worst = {}
    for n in trained:
        if n.endswith("box_predictor.det.bias"):
            continue   # a per-image soft-max over the proposals: det's bias cancels, the gradient is rounding noise
        g = got[n].grad
        assert g is not None, n
        if n.endswith("box_head.fc1.weight"):
            g = model.roi_heads.box_head._hwc_cols(g, False)
        g0 = p[n].grad
        d = g.detach().cpu().double() - g0.double()
        worst[n] = (d.norm() / (g0.double().norm() + 1e-12)).item()
    print(worst)
    bar = {n: (5e-3 if n == res5 else grad_bar) for n in trained}
    bad = {n: v for n, v in worst.items() if v > bar[n]}
    assert not bad, bad


def test_frozen_backbone_runs_no_pooling_backward(cuda):
    """FREEZE_AT 5: the pooled rows carry no gradient, so the ROIPool backward never runs (counted through the
    library's call log) and no backbone parameter gets a gradient; every branch clusters and takes its loss on the
    device."""
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
    assert "jtsm_roi_pool_forward_f32" in names_fwd
    assert "jtsm_roi_pool_backward_f32" not in names
    for n in ("jtsm_pcl_softmax_f32", "jtsm_pcl_cluster_f32", "jtsm_pcl_loss_forward_f32"):
        assert names_fwd.count(n) == 3, (n, names_fwd.count(n))
    assert names.count("jtsm_pcl_loss_backward_f32") == 3
    assert all(q.grad is None for q in model.backbone.parameters())


def test_inference_matches_cpu_composition(cuda):
    from model_util import to_batched_inputs
    from oracle import inference as OI

    p = _params()
    batch = _batch(R=200)
    with torch.no_grad():
        _, _, Z, counts = _cpu_logits(p, batch)
        avg = sum(torch.softmax(z, dim=1) for z in Z) / 3
        scores0 = torch.cat((avg[:, 1:], avg[:, :1]), dim=1)          # pcl_bg: the background behind the classes
    model = _model(p)
    model.roi_heads.box_refinery[-1].test_score_thresh = 1e-5
    model.roi_heads.box_refinery[-1].test_nms_thresh = 0.3
    model.eval()
    inputs = to_batched_inputs(batch)
    results, all_scores, all_boxes = model.inference(inputs, do_postprocess=False)
    out = model(inputs)
    assert len(out) == 2 and set(out[0]) == {"instances"}
    for i, (inst, sc, bx, img) in enumerate(zip(results, all_scores, all_boxes, batch["images"])):
        s0 = scores0.split(counts)[i]
        assert sc[0].shape == s0.shape
        assert torch.allclose(sc[0].cpu(), s0, rtol=1e-4, atol=1e-5 * float(s0.max()))
        # zero deltas: every class's box is the proposal, up to apply_deltas' centre / size round trip in float32
        # (coordinates <= 256: an ulp is 3e-5, a handful of roundings)
        assert torch.allclose(bx[0].cpu().view(len(s0), 20, 4)[:, 7], batch["boxes"][i], rtol=0, atol=2e-4)
        # the product's own selection re-derived by the oracle NMS from the product's scores and boxes
        want = OI.fast_rcnn_inference_single_image(bx[0].cpu(), sc[0].cpu(), tuple(img.shape[-2:]), 1e-5, 0.3, 100)
        assert torch.equal(inst.pred_classes.cpu(), want["classes"]) and torch.equal(inst.pred_inds.cpu(), want["rows"])
        assert len(inst) > 0
