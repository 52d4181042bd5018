"""GPU suite (pytest -m gpu): OICR + MIST end to end — GeneralizedRCNNWSL + OICRROIHeads + WSDDNOutputLayers + four
regressing OICROutputLayers branches on the shipped configuration (tests/golden/configs/oicr_mist_WSR_18_DC5_1x.yaml,
DAN narrowed to 512) against a CPU composition built as tests/test_hip_pcl_model.py builds its own: the oracle's
ResNet-WS v2 dilated-C5 backbone, the ROIPool restatement, the DAN as F.linear + ReLU, cls / det and the MIL scores of
oracle/model.py, and per branch the MIST labelling of tests/mist_ref.py with the DEVICE's mined rows frozen in (which
proposals are pseudo ground truth — a choice among near-equal scores that hangs on the last bit of a GEMM; their boxes
and scores are recomputed on the CPU from the device's previous-branch logits) followed by the oracle's weighted
cross-entropy and the weighted smooth-L1 (beta 1) loss in torch autograd.  Branch 0's terms carry the factor 3.
Bars are the PCL model test's: loss 1e-4; gradients 2e-4 in f32 and 1e-3 in bf16x3 (L2 relative)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mist_ref as MR
import roi_pool_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from jtsm_amd.config import add_wsl_config, get_cfg  # noqa: E402
from jtsm_amd.modeling import build_model  # noqa: E402

CFG = os.path.join(GOLDEN, "configs", "oicr_mist_WSR_18_DC5_1x.yaml")
DAN = 512
NB = 4
CLS = ["roi_heads.box_refinery_%d.cls_score" % k for k in range(NB)]
BOX = ["roi_heads.box_refinery_%d.bbox_pred" % k for k in range(NB)]
HEAD = ["roi_heads.box_head.fc1", "roi_heads.box_head.fc2", "roi_heads.box_predictor.cls",
        "roi_heads.box_predictor.det"] + CLS + BOX


def _cfg(mist=True):
    cfg = get_cfg()
    add_wsl_config(cfg)
    cfg.merge_from_file(CFG)
    cfg.MODEL.DEVICE = "cuda"
    cfg.MODEL.ROI_BOX_HEAD.DAN_DIM = [DAN, DAN]
    cfg.WSL.REFINE_MIST = mist
    return cfg


def _params(seed=11):
    from oracle import model as OM
    p = OM.init_params_dc5(seed=seed, depth=18, nt=20, ns=2, dan_dims=(DAN, DAN), input_gain=1.0 / 64)
    p = {k: v for k, v in p.items() if not k.startswith("roi_heads.") or k.startswith("roi_heads.box_head.")}
    g = torch.Generator().manual_seed(seed + 1)
    for n in ("cls", "det"):
        p["roi_heads.box_predictor.%s.weight" % n] = torch.randn(20, DAN, generator=g) * 0.05
        p["roi_heads.box_predictor.%s.bias" % n] = torch.randn(20, generator=g) * 0.01
    for k in range(NB):
        p[CLS[k] + ".weight"] = torch.randn(21, DAN, generator=g) * 0.05
        p[CLS[k] + ".bias"] = torch.randn(21, generator=g) * 0.01
        p[BOX[k] + ".weight"] = torch.randn(80, DAN, generator=g) * 0.01
        p[BOX[k] + ".bias"] = torch.randn(80, generator=g) * 0.01
    return p


def _batch(seed=77, R=300):
    from oracle import model as OM
    return OM.synthetic_batch(seed, B=2, size=256, R=R, sp_block=8, n_stuff=1, nt=20, ns=2, cluster=0.7, objects=6)


def _model(p, mist=True):
    model = build_model(_cfg(mist))
    missing, unexpected = model.load_state_dict({k: v.detach() for k, v in p.items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    model.roi_heads.box_head.dropout_p = 0.0
    return model


def _cpu_logits(p, batch):
    """CPU composition of the forward up to the logits: (cls, det, [branch logits], [branch deltas], counts)."""
    from oracle import model as OM
    x = OM.preprocess(p, batch["images"], 8)
    feat = OM.wsr_v2_dc5(p, x, 18)
    counts = [len(b) for b in batch["boxes"]]
    rois = torch.cat([torch.cat([torch.full((n, 1), float(i)), b], 1) for i, (n, b) in enumerate(zip(counts, batch["boxes"]))])
    _, arg = ref.forward(feat.detach().numpy(), rois.numpy(), 0.125, 7, 7)
    arg = torch.from_numpy(arg.astype(np.int64)).flatten(2)
    b = rois[:, 0].to(torch.int64)
    flat = feat.flatten(2)
    cidx = torch.arange(flat.shape[1])
    pooled = flat[b[:, None, None], cidx[None, :, None], arg.clamp(min=0)] * (arg >= 0).to(flat.dtype)
    scale = torch.cat([o + 1 for o in batch["objectness"]])
    h = (pooled * scale.view(-1, 1, 1)).flatten(1)
    for n in ("fc1", "fc2"):
        h = F.relu(F.linear(h, p["roi_heads.box_head.%s.weight" % n], p["roi_heads.box_head.%s.bias" % n]))
    lin = lambda name: F.linear(h, p[name + ".weight"], p[name + ".bias"])  # noqa: E731
    return (lin("roi_heads.box_predictor.cls"), lin("roi_heads.box_predictor.det"), [lin(n) for n in CLS],
            [lin(n) for n in BOX], counts)


def _smooth_l1_losses(z, d, labels, w, prop, gt, beta):
    """oracle.model.oicr_losses with smooth_l1_loss(beta) in the box term."""
    from oracle import model as OM
    kc = z.shape[1] - 1
    valid = (w > 1e-12).to(w.dtype).sum()
    ce = F.cross_entropy(z, labels, reduction="none", ignore_index=-1)
    fg = torch.nonzero((labels >= 0) & (labels < kc))[:, 0]
    cols = 4 * labels[fg][:, None] + torch.arange(4)
    n = (d[fg[:, None], cols] - OM.box_deltas(prop, gt)[fg]).abs()
    l = torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
    return (ce * w).sum() / valid, (l * w[fg, None]).sum() / labels.numel()


def _frozen_targets(aux, k, batch, counts):
    """Per image the restatement's target list of branch k with the device's rows: boxes and scores recomputed on the
    CPU from the device's previous-branch predictions."""
    from oracle import model as OM
    rows, num, cls = (aux["pgt_rows_r%d" % k].cpu().long(), aux["pgt_num_r%d" % k].cpu().long(),
                      aux["pgt_classes_r%d" % k].cpu().long())
    out, lo = [], 0
    for i, n in enumerate(counts):
        r, c = rows[i, :num[i]], cls[i, :num[i]]
        b = batch["boxes"][i]
        if k == 0:
            boxes, scores = b[r], aux["mil_scores"].cpu()[lo:lo + n][r, c]
        else:
            z, d = aux["logits_r%d" % (k - 1)].cpu()[lo:lo + n], aux["deltas_r%d" % (k - 1)].cpu()[lo:lo + n]
            boxes = OM.apply_deltas(d, b).view(n, 20, 4)[r, c]
            scores = torch.softmax(z, dim=-1)[r, c]
        out.append(dict(boxes=boxes, classes=c, scores=scores, weights=scores))
        lo += n
    return out


@pytest.fixture
def conv_math(request):
    from jtsm_amd.layers import conv as K
    old = K.MATH
    K.set_math(request.param)
    yield request.param
    K.set_math(old)


STEP_CASES = [("f32", 1e-4, 2e-4), ("bf16x3", 1e-4, 1e-3)]


@pytest.mark.parametrize("conv_math,loss_bar,grad_bar", STEP_CASES, indirect=["conv_math"], ids=[m for m, _, _ in STEP_CASES])
def test_training_step_matches_cpu_composition(cuda, conv_math, loss_bar, grad_bar):
    from model_util import to_batched_inputs
    from oracle import model as OM

    p = _params()
    batch = _batch()
    trained = [k for k in p if any(k.startswith(h + ".") for h in HEAD)]
    model = _model(p)
    model.train()
    losses = model(to_batched_inputs(batch))
    keys = {"loss_cls"} | {"loss_cls_r%d" % k for k in range(NB)} | {"loss_box_reg_r%d" % k for k in range(NB)}
    assert set(losses) == keys
    sum(losses.values()).backward()
    aux = model.roi_heads.aux

    for k in trained:
        p[k].requires_grad_(True)
    C, D, Z, DL, counts = _cpu_logits(p, batch)
    probs = OM.mil_image_probs(OM.mil_scores(C, D, counts), counts)
    _, _, oh = OM.image_labels(batch["gt_classes"], batch["sem_seg"], 20, 2)
    want = {"loss_cls": F.binary_cross_entropy(probs, oh[:, :20], reduction="mean")}
    prop = torch.cat(batch["boxes"])
    for k in range(NB):
        tg = _frozen_targets(aux, k, batch, counts)
        assert all(len(t["classes"]) >= 1 for t in tg)
        labs = [MR.label(b, t, 20) for b, t in zip(batch["boxes"], tg)]
        labels = torch.cat([l["classes"] for l in labs])
        assert torch.equal(aux["labels_r%d" % k].cpu().long(), labels), k          # bit-equal labels
        assert int((labels < 20).sum()) > 0
        lc, lb = _smooth_l1_losses(Z[k], DL[k], labels, torch.cat([l["weights"] for l in labs]), prop,
                                   torch.cat([l["boxes"] for l in labs]), 1.0)
        factor = 3.0 if k == 0 else 1.0                                            # (:423-424, :443-444)
        want["loss_cls_r%d" % k], want["loss_box_reg_r%d" % k] = lc * factor, lb * factor
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
    bad = {n: v for n, v in worst.items() if v > grad_bar}
    assert not bad, bad


def test_branch_zero_carries_the_factor_three_and_top1_labels_without_mist(cuda):
    """The same weights with REFINE_MIST off: branch 0's labels are mine_top1 + match_label's, and its loss without the
    factor; with MIST on and the same labels frozen the factor is exactly 3 — checked through the loss layer itself."""
    from model_util import to_batched_inputs
    from jtsm_amd.layers.mining import match_label, mine_top1, row_lse
    from jtsm_amd.modeling.roi_heads.roi_heads_jtsm import class_lists

    p = _params()
    batch = _batch()
    model = _model(p, mist=False)
    model.train()
    inputs = to_batched_inputs(batch)
    losses = model(inputs)
    heads = model.roi_heads
    aux = heads.aux
    counts = [len(b) for b in batch["boxes"]]
    off = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32, device=cuda)
    boxes = torch.cat(batch["boxes"]).to(cuda)
    cls, cnt = class_lists(heads.gt_classes_img_oh)
    for k in range(NB):
        if k == 0:
            pg = mine_top1(aux["mil_scores"], boxes, off, cls, cnt, aux["img_probs"])
        else:
            z = aux["logits_r%d" % (k - 1)]
            pg = mine_top1(z, boxes, off, cls, cnt, aux["img_probs"], lse=row_lse(z), deltas=aux["deltas_r%d" % (k - 1)])
        lab = match_label(boxes, off, pg, cls, cnt, 20)
        assert torch.equal(aux["labels_r%d" % k], lab["labels"]), k
        assert torch.equal(aux["pgt_rows_r%d" % k], pg["idx"]), k
    # MIST on: branch 0's two terms are 3 x what its loss layer returns for the recorded labels
    model = _model(p, mist=True)
    model.train()
    losses = model(inputs)
    heads = model.roi_heads
    aux = heads.aux
    from jtsm_amd.layers.mist import mine_top_p, top_p_counts
    top_t, t_max = top_p_counts(counts, 0.15, cuda)
    pg = mine_top_p(aux["mil_scores"], boxes, off, cls, cnt, top_t, t_max)
    assert torch.equal(pg["rows"], aux["pgt_rows_r0"]) and torch.equal(pg["num"], aux["pgt_num_r0"])
    lab = match_label(boxes, off, pg, pg["classes"], pg["num"], 20)
    plain = heads.box_refinery[0].losses((aux["logits_r0"], aux["deltas_r0"]), boxes, lab["labels"], lab["boxes"],
                                         lab["weights"])
    for name, v in plain.items():
        assert torch.equal(losses[name].detach(), v.detach() * 3), name


def test_inference_matches_cpu_composition(cuda):
    from model_util import to_batched_inputs
    from oracle import inference as OI

    p = _params()
    batch = _batch(R=200)
    with torch.no_grad():
        _, _, Z, DL, counts = _cpu_logits(p, batch)
        probs0, boxes0 = OI.predict_K(Z, DL, torch.cat(batch["boxes"]))
    model = _model(p)
    model.roi_heads.box_refinery[-1].test_score_thresh = 1e-5
    model.roi_heads.box_refinery[-1].test_nms_thresh = 0.3
    model.eval()
    inputs = to_batched_inputs(batch)
    results, all_scores, all_boxes = model.inference(inputs, do_postprocess=False)
    out = model(inputs)
    assert len(out) == 2 and set(out[0]) == {"instances"}
    for i, (inst, sc, bx, img) in enumerate(zip(results, all_scores, all_boxes, batch["images"])):
        s0, b0 = probs0.split(counts)[i], boxes0.split(counts)[i]
        assert sc[0].shape == s0.shape and bx[0].shape == b0.shape
        assert torch.allclose(sc[0].cpu(), s0, rtol=1e-4, atol=1e-5 * float(s0.max()))
        assert torch.allclose(bx[0].cpu(), b0, rtol=1e-4, atol=1e-2)
        # the product's own selection re-derived by the oracle NMS from the product's scores and boxes
        want = OI.fast_rcnn_inference_single_image(bx[0].cpu(), sc[0].cpu(), tuple(img.shape[-2:]), 1e-5, 0.3, 100)
        assert torch.equal(inst.pred_classes.cpu(), want["classes"]) and torch.equal(inst.pred_inds.cpu(), want["rows"])
        assert len(inst) > 0
