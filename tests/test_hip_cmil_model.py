"""GPU suite (pytest -m gpu): C-MIL end to end — GeneralizedRCNNWSL + CMILROIHeads + WSDDNOutputLayers(cmil) + three
non-regressing OICROutputLayers branches on the shipped configuration (tests/golden/configs/cmil_WSR_18_DC5_1x.yaml, DAN
narrowed to 512) against a CPU composition built as tests/test_hip_oicr_model.py builds its own: the oracle's ResNet-WS
v2 dilated-C5 backbone, the ROILoopPool restatement, the DAN as F.linear + ReLU, cls(box) / det(frame) - det(context),
then
  * the restatement's ROIMerge (tests/cmil_ref.py) fed the device's score sums: its I must equal the device's and is
    then used in torch autograd (MC = sum over the members of C / IC), the MIL scores of the merged bags, BCE (mean);
  * per branch the restatement's ROILabel with the DEVICE's seeds and visiting order frozen in (which proposal is a
    seed is a choice among near-equal scores that hangs on the last bit of a GEMM; the order is drawn on the device),
    scores and image probabilities taken from the device; its labels must equal the device's, then the oracle's
    weighted cross-entropy.
Bars are the OICR model test's: loss 1e-4; gradients 2e-4 in f32 and 1e-3 in bf16x3 (L2 relative)."""
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cmil_ref as CR
import roi_loop_pool_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from jtsm_amd.config import add_wsl_config, get_cfg  # noqa: E402
from jtsm_amd.modeling import build_model  # noqa: E402

CFG = os.path.join(GOLDEN, "configs", "cmil_WSR_18_DC5_1x.yaml")
DAN = 512
NB = 3
CLS = ["roi_heads.box_refinery_%d.cls_score" % k for k in range(NB)]
BOX = ["roi_heads.box_refinery_%d.bbox_pred" % k for k in range(NB)]
HEAD = ["roi_heads.box_head.fc1", "roi_heads.box_head.fc2", "roi_heads.box_predictor.cls",
        "roi_heads.box_predictor.det"] + CLS
CUR_ITER = 2500        # lambda = getlambda(2, 40) = 0.64: cliques of several sizes


def _cfg():
    cfg = get_cfg()
    add_wsl_config(cfg)
    cfg.merge_from_file(CFG)
    cfg.MODEL.DEVICE = "cuda"
    # the oracle's backbone (resnet_wsl_v2.py); the shipped file names v1, whose pools sit one block later
    cfg.MODEL.BACKBONE.NAME = "build_wsl_resnet_v2_backbone"
    cfg.MODEL.ROI_BOX_HEAD.DAN_DIM = [DAN, DAN]
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
        p[BOX[k] + ".weight"] = torch.randn(80, DAN, generator=g) * 0.01     # (built, unused: REFINE_REG is off)
        p[BOX[k] + ".bias"] = torch.randn(80, generator=g) * 0.01
    return p


def _batch(seed=77, R=300):
    from oracle import model as OM
    return OM.synthetic_batch(seed, B=2, size=256, R=R, sp_block=8, n_stuff=1, nt=20, ns=2, cluster=0.7, objects=6)


def _model(p):
    model = build_model(_cfg())
    missing, unexpected = model.load_state_dict({k: v.detach() for k, v in p.items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    model.roi_heads.box_head.dropout_p = 0.0
    model.roi_heads.box_predictor.roi_merge.cur_iter = CUR_ITER
    return model


def _cpu_logits(p, batch):
    """CPU composition of the forward up to the logits: (C, D, [branch logits], counts)."""
    from oracle import model as OM
    x = OM.preprocess(p, batch["images"], 8)
    feat = OM.wsr_v2_dc5(p, x, 18)
    counts = [len(b) for b in batch["boxes"]]
    rois = torch.cat([torch.cat([torch.full((n, 1), float(i)), b], 1) for i, (n, b) in enumerate(zip(counts, batch["boxes"]))])
    _, arg = ref.forward(feat.detach().numpy(), rois.numpy(), 0.125, 7, 7)
    arg = torch.from_numpy(arg.astype(np.int64)).flatten(2)                       # (3R, C, 49)
    R = rois.shape[0]
    b = rois[:, 0].to(torch.int64).repeat(3)
    flat = feat.flatten(2)
    cidx = torch.arange(flat.shape[1])
    pooled = flat[b[:, None, None], cidx[None, :, None], arg.clamp(min=0)] * (arg >= 0).to(flat.dtype)
    scale = torch.cat([o + 1 for o in batch["objectness"]]).repeat(3)
    h = (pooled * scale.view(-1, 1, 1)).flatten(1)
    for n in ("fc1", "fc2"):
        h = F.relu(F.linear(h, p["roi_heads.box_head.%s.weight" % n], p["roi_heads.box_head.%s.bias" % n]))
    lin = lambda name, t: F.linear(t, p[name + ".weight"], p[name + ".bias"])  # noqa: E731
    det = "roi_heads.box_predictor.det"
    return (lin("roi_heads.box_predictor.cls", h[:R]), lin(det, h[R:2 * R]) - lin(det, h[2 * R:]),
            [lin(n, h[:R]) for n in CLS], counts)


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
    assert set(losses) == {"loss_cls"} | {"loss_cls_r%d" % k for k in range(NB)}
    sum(losses.values()).backward()
    aux = model.roi_heads.aux
    assert aux["pooled_rows"] == 3 * 600

    for k in trained:
        p[k].requires_grad_(True)
    C, D, Z, counts = _cpu_logits(p, batch)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    prop = torch.cat(batch["boxes"])

    # ---- the merge: the restatement on the device's score sums gives the device's cliques
    lam = CR.getlambda(CUR_ITER, 1250, 40)
    assert aux["merge_lambda"] == float(lam) and 0.6 < lam < 0.7
    merged = CR.roi_merge(aux["merge_scores"].cpu().numpy(), prop.numpy(), C.detach().numpy(), D.detach().numpy(), offsets, lam)
    assert np.array_equal(aux["merge_rows"].cpu().numpy(), merged["I"])
    assert np.array_equal(aux["merge_counts"].cpu().numpy(), merged["IC"])
    assert np.array_equal(aux["merged_offsets"].cpu().numpy(), merged["merged_offsets"])
    live = int(merged["merged_offsets"][-1])
    sizes = merged["IC"][:live]
    print("merged rows %d of 600, clique sizes up to %d" % (live, sizes.max()))
    assert live < 600 and sizes.max() >= 2 and sizes.min() == 1                     # something merged, something did not
    I = torch.from_numpy(merged["I"].astype(np.int64))
    cnt = torch.from_numpy(merged["IC"].astype(np.float32))[I][:, None]
    MC = torch.zeros(live, 20).index_add(0, I, C / cnt)
    MD = torch.zeros(live, 20).index_add(0, I, D / cnt)
    mcounts = np.diff(merged["merged_offsets"]).tolist()
    probs = OM.mil_image_probs(OM.mil_scores(MC, MD, mcounts), mcounts)
    _, _, oh = OM.image_labels(batch["gt_classes"], batch["sem_seg"], 20, 2)
    want = {"loss_cls": F.binary_cross_entropy(probs, oh[:, :20], reduction="mean")}
    # (sanity, not a bar: the image probabilities are the merged bags', the scores the proposals' own)
    assert torch.allclose(aux["img_probs"].cpu(), probs.detach(), rtol=1e-3, atol=1e-6)
    assert torch.allclose(aux["mil_scores"].cpu(), OM.mil_scores(C, D, counts).detach(), rtol=1e-2, atol=1e-6)

    # ---- the branches: the device's seeds and order frozen into the restatement's labelling
    things = [torch.unique(g).tolist() for g in batch["gt_classes"]]
    CW = aux["img_probs"].cpu().numpy()
    for k in range(NB):
        S = (aux["mil_scores"] if k == 0 else torch.softmax(aux["logits_r%d" % (k - 1)], dim=1)).cpu().numpy()
        seeds, num = aux["seed_rows_r%d" % k].cpu().numpy(), aux["seed_num_r%d" % k].cpu().numpy()
        perm = aux["perm_r%d" % k].cpu().numpy()
        labels, weights = [], []
        for i, n in enumerate(counts):
            lo, hi = offsets[i], offsets[i + 1]
            assert int(num[i]) == len(things[i]) and sorted(perm[lo:hi].tolist()) == list(range(n))
            rows = seeds[i, :num[i]].tolist()
            assert len(set(rows)) == len(rows)
            frozen = (rows, things[i], [S[lo:hi][r, c] for r, c in zip(rows, things[i])])
            out = CR.roi_label_image(S[lo:hi], batch["boxes"][i].numpy(), things[i], CW[i], perm[lo:hi], 0.6, 0.4, 0.1, 32,
                                     96, 1, num_classes=20, seeds=frozen)
            labels.append(out["labels"])
            weights.append(out["weights"])
        labels, weights = np.concatenate(labels), np.concatenate(weights)
        assert np.array_equal(aux["labels_r%d" % k].cpu().numpy(), labels), k       # bit-equal labels
        assert np.array_equal(aux["weights_r%d" % k].cpu().numpy(), weights), k
        assert 0 < int((weights > 0).sum()) <= 2 * (33 + 97) and int((labels == 20).sum()) > 0
        w = torch.from_numpy(weights)
        ce = F.cross_entropy(Z[k], torch.from_numpy(labels.astype(np.int64)), reduction="none")
        want["loss_cls_r%d" % k] = (ce * w).sum() / (w > 1e-12).to(w.dtype).sum()
    sum(want.values()).backward()
    for k, v in want.items():
        a, b = float(losses[k].detach()), float(v.detach())
        print("%s: device %.8g cpu %.8g rel %.3g" % (k, a, b, abs(a - b) / abs(b)))
        assert abs(a - b) <= loss_bar * abs(b) + 1e-7, (k, a, b)
    got = dict(model.named_parameters())
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
    print(worst)
    bad = {n: v for n, v in worst.items() if v > grad_bar}
    assert not bad, bad


def test_cur_iter_advances_and_moves_lambda_without_a_host_round_trip(cuda):
    from model_util import to_batched_inputs
    from jtsm_amd.layers import cmil as layer
    from jtsm_amd.modeling.roi_heads import roi_heads_cmil as heads
    from jtsm_amd.modeling.roi_heads.fast_rcnn_wsddn import WSDDNOutputLayers

    model = _model(_params())
    merge = model.roi_heads.box_predictor.roi_merge
    inputs = to_batched_inputs(_batch(R=64))
    model.train()
    merge.cur_iter = 0
    model(inputs)
    aux = model.roi_heads.aux
    assert merge.cur_iter == 1 and aux["merge_lambda"] == 0.0
    # lambda 0: the 64 rows of an image fall into windows of 40 by rank
    assert aux["merged_offsets"].cpu().tolist() == [0, 2, 4]
    first = aux["merged_offsets"]
    model(inputs)
    aux = model.roi_heads.aux
    assert merge.cur_iter == 2 and 0.0 < aux["merge_lambda"] == float(CR.getlambda(1, 1250, 40)) < 0.1
    merge.cur_iter = 50000                                                            # settable: a resumed run's last step
    model(inputs)
    aux = model.roi_heads.aux
    assert merge.cur_iter == 50001 and aux["merge_lambda"] == 1.0
    assert int(aux["merged_offsets"][-1]) > 4                                         # only identical boxes merge now
    # the clique counts stayed on the device: device tensors in, device tensors out, and nothing on the path reads back
    for t in (first, aux["merged_offsets"], aux["merge_rows"], aux["merge_counts"], aux["perm_r0"], aux["seed_num_r0"]):
        assert t.is_cuda and t.dtype == torch.int32
    path = [inspect.getsource(layer), inspect.getsource(heads.CMILROIHeads._forward_box),
            inspect.getsource(WSDDNOutputLayers.score_and_loss_cmil)]
    for src in path:
        for word in (".item(", ".cpu(", ".tolist(", ".numpy(", "synchronize", "nonzero"):
            assert word not in src, word
    model.eval()
    with torch.no_grad():
        model(inputs)
    assert merge.cur_iter == 50001                                                    # inference does not count


def test_inference_matches_cpu_composition(cuda):
    from model_util import to_batched_inputs
    from oracle import inference as OI

    p = _params()
    batch = _batch(R=200)
    with torch.no_grad():
        _, _, Z, counts = _cpu_logits(p, batch)
        zeros = [torch.zeros(Z[0].shape[0], 80) for _ in Z]
        probs0, boxes0 = OI.predict_K(Z, zeros, torch.cat(batch["boxes"]))
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
        assert sc[0].shape == s0.shape == (200, 21) and bx[0].shape == b0.shape == (200, 80)
        assert torch.allclose(sc[0].cpu(), s0, rtol=1e-4, atol=1e-5 * float(s0.max()))
        assert torch.allclose(bx[0].cpu(), b0, rtol=1e-4, atol=1e-2)
        # the product's own selection re-derived by the oracle NMS from the product's scores and boxes
        want = OI.fast_rcnn_inference_single_image(bx[0].cpu(), sc[0].cpu(), tuple(img.shape[-2:]), 1e-5, 0.3, 100)
        assert torch.equal(inst.pred_classes.cpu(), want["classes"]) and torch.equal(inst.pred_inds.cpu(), want["rows"])
        assert len(inst) > 0
