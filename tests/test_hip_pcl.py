"""GPU suite (pytest -m gpu): the operators PCL adds — the ROIPool kernel (csrc/roi_pool.hip) through the
jtsm_amd.layers / ROIPooler surfaces against tests/roi_pool_ref.py, and the device-side proposal clustering and PCL
loss (csrc/pcl.hip, layers/pcl.py) against tests/pcl_ref.py.

Bars: ROIPool forward values and argmax bit-exact in both layouts, backward within 1e-6 (relative to the largest
gradient) of the restatement's scatter-add, bit-identical across calls, bit-identical to the float32 sum taken in the
documented order, and unchanged by rois that name no image.  Clustering: integer tables bit-exact, float
tables within 1e-6 relative (fp32 roundings of fp64 sums against exactly summed ones), two runs identical.  Loss and
logit gradient: 1e-4 of the largest reference entry, the bar tests/test_hip_losses.py uses for OICR."""
import zlib

import numpy as np
import pytest
import torch

import pcl_ref
import roi_pool_ref as ref
from conftest import load_cases
from test_hip_contextlocnet import _feat, _rois, _rows, _sum_in_order
from test_hip_losses import rel_close

pytestmark = pytest.mark.gpu

from jtsm_amd.layers import ROIPool  # noqa: E402
from jtsm_amd.layers.pcl import pcl_cluster, pcl_loss, pcl_softmax  # noqa: E402
from jtsm_amd.layers.roi_pool import roi_pool_backward, roi_pool_forward  # noqa: E402
from jtsm_amd.modeling.poolers import ROIPooler  # noqa: E402
from jtsm_amd.structures import Boxes  # noqa: E402

CL = torch.channels_last


# ---------------------------------------------------------------------------------------------------------- ROIPool
def _gpu_forward(x, rois, scale, P, cuda, nhwc):
    xt = torch.from_numpy(x).to(cuda)
    if nhwc:
        xt = xt.contiguous(memory_format=CL)
    out, arg = roi_pool_forward(xt, torch.from_numpy(rois).to(cuda), scale, P, P)
    if nhwc and out.numel():
        assert out.is_contiguous(memory_format=CL) and arg.is_contiguous(memory_format=CL)
    return out.cpu().numpy(), arg.cpu().numpy()


CASES = [("random", "relu", 1, 16, 48), ("clustered", "relu", 2, 64, 60), ("large", "relu", 2, 8, 20),
         ("borders", "relu", 2, 12, 40), ("degenerate", "relu", 1, 8, 30), ("random", "zero", 2, 8, 10),
         ("random", "negative", 1, 4, 10), ("clustered", "signed", 3, 3, 25), ("random", "relu", 2, 8, 0),
         ("stray", "relu", 2, 8, 40)]


@pytest.mark.parametrize("nhwc", [True, False], ids=["nhwc", "nchw"])
@pytest.mark.parametrize("kind,feat,B,C,R", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_roi_pool_forward_matches_restatement_bit_exact(cuda, kind, feat, B, C, R, nhwc):
    rng = np.random.default_rng(zlib.crc32(repr((kind, feat, B, C, R)).encode()))
    H, W, stride, P = 20, 24, 8, 7
    x = _feat(rng, B, C, H, W, feat)
    rois = _rois(kind, rng, B, H, W, stride, R)
    if kind == "large" and R:                      # out of the map altogether: every bin empty
        rois[:3, 1:] += 10 * W * stride
    want, want_arg = ref.forward(x, rois, 1.0 / stride, P, P)
    got, got_arg = _gpu_forward(x, rois, 1.0 / stride, P, cuda, nhwc)
    assert got.shape == (R, C, P, P)
    np.testing.assert_array_equal(got_arg, want_arg)
    np.testing.assert_array_equal(got, want)
    if kind == "stray":                            # a roi naming no image pools nothing
        bad = (rois[:, 0] < 0) | (rois[:, 0] >= B)
        assert bad.sum() == 10 and (got[bad] == 0).all() and (got_arg[bad] == -1).all()
        assert (got_arg[~bad] >= 0).any()


def test_roi_pool_flagship_channels_and_module(cuda):
    rng = np.random.default_rng(11)
    B, C, H, W = 2, 512, 24, 20
    x = _feat(rng, B, C, H, W)
    rois = np.concatenate([_rois("clustered", rng, B, H, W, 8, 24), _rois("borders", rng, B, H, W, 8, 8)])
    want, want_arg = ref.forward(x, rois, 0.125, 7, 7)
    got, got_arg = _gpu_forward(x, rois, 0.125, 7, cuda, True)
    np.testing.assert_array_equal(got_arg, want_arg)
    np.testing.assert_array_equal(got, want)
    m = ROIPool((7, 7), 0.125)
    assert repr(m) == "ROIPool(output_size=(7, 7), spatial_scale=0.125)"
    half = m(torch.from_numpy(x).to(cuda).half(), torch.from_numpy(np.round(rois)).to(cuda).half())
    want16, _ = ref.forward(x.astype(np.float16).astype(np.float32), np.round(rois), 0.125, 7, 7)
    assert half.dtype == torch.float16
    np.testing.assert_array_equal(half.cpu().numpy(), want16.astype(np.float16))


def test_roi_pooler_single_and_multi_level(cuda):
    rng = np.random.default_rng(9)
    B, C = 2, 8
    feats_np = [_feat(rng, B, C, 64 // s, 64 // s) for s in (4, 8)]
    boxes = [np.abs(_rois("random", rng, 1, 8, 8, 8, n)[:, 1:]) for n in (7, 5)]
    box_lists = [Boxes(torch.from_numpy(b).to(cuda)) for b in boxes]
    feats = [torch.from_numpy(f).to(cuda).contiguous(memory_format=CL) for f in feats_np]
    p1 = ROIPooler(7, (1.0 / 8,), 0, "ROIPool")
    out1 = p1([feats[1]], box_lists).cpu().numpy()
    rois = np.concatenate([np.concatenate([np.full((len(b), 1), i, np.float32), b], 1) for i, b in enumerate(boxes)])
    want1, _ = ref.forward(feats_np[1], rois, 1.0 / 8, 7, 7)
    np.testing.assert_array_equal(out1, want1)
    p2 = ROIPooler(7, (1.0 / 4, 1.0 / 8), 0, "ROIPool", canonical_box_size=16, canonical_level=3)
    level_ids = [torch.from_numpy(np.arange(len(b)) % 2).to(cuda) for b in boxes]
    out2 = p2(feats, box_lists, level_ids=level_ids).cpu().numpy()
    lvl = np.concatenate([np.arange(len(b)) % 2 for b in boxes])
    assert out2.shape == (len(rois), C, 7, 7)
    for level, scale in ((0, 0.25), (1, 0.125)):
        idx = np.nonzero(lvl == level)[0]
        want, _ = ref.forward(feats_np[level], rois[idx], scale, 7, 7)
        np.testing.assert_array_equal(out2[idx], want)


@pytest.mark.parametrize("C,nhwc", [(512, True), (6, True), (4, False)], ids=["c512-nhwc", "c6-nhwc", "c4-nchw"])
def test_roi_pool_backward_matches_restatement_and_is_reproducible(cuda, C, nhwc):
    rng = np.random.default_rng(C)
    B, H, W = 2, 20, 24
    x = _feat(rng, B, C, H, W)
    rois = np.concatenate([_rois("clustered", rng, B, H, W, 8, 20), _rois("borders", rng, B, H, W, 8, 6),
                           _rois("degenerate", rng, B, H, W, 8, 4), _rois("large", rng, B, H, W, 8, 2),
                           _rois("stray", rng, B, H, W, 8, 12)])
    R = len(rois)
    g = rng.standard_normal((R, C, 7, 7)).astype(np.float32)
    _, arg = ref.forward(x, rois, 0.125, 7, 7)
    want = ref.backward(g, rois, arg, B, C, H, W)
    xt = torch.from_numpy(x).to(cuda)
    if nhwc:
        xt = xt.contiguous(memory_format=CL)
    xt.requires_grad_(True)
    rt = torch.from_numpy(rois).to(cuda)
    out = ROIPool((7, 7), 0.125)(xt, rt)
    gt = torch.from_numpy(g).to(cuda).contiguous(memory_format=CL if nhwc else torch.contiguous_format)
    out.backward(gt)
    got = xt.grad.cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6 * float(np.abs(want).max()))
    _, argt = roi_pool_forward(xt.detach(), rt, 0.125, 7, 7)
    again = roi_pool_backward(gt, rt, argt, 0.125, 7, 7, B, C, H, W).cpu().numpy()
    np.testing.assert_array_equal(again, got)
    # the documented order, in float32: rois ascending, bins ph outer, pw inner
    np.testing.assert_array_equal(argt.cpu().numpy(), arg)
    ordered = _sum_in_order(_rows(arg, R).reshape(-1, C), _rows(g, R).reshape(-1, C), np.repeat(rois[:, 0], 49),
                            B, C, H, W)
    np.testing.assert_array_equal(got, ordered)
    # the rois that name no image removed from rois, argmax and grad: the same bits
    keep = torch.from_numpy((rois[:, 0] >= 0) & (rois[:, 0] < B)).to(cuda)
    assert 0 < int(keep.sum()) < R
    without = roi_pool_backward(gt[keep], rt[keep], argt[keep], 0.125, 7, 7, B, C, H, W, nhwc=nhwc).cpu().numpy()
    np.testing.assert_array_equal(without, got)


def test_roi_pool_without_rois_is_zero(cuda):
    x = torch.rand(2, 8, 6, 6, device=cuda).contiguous(memory_format=CL).requires_grad_(True)
    out = ROIPool((7, 7), 0.125)(x, torch.zeros((0, 5), device=cuda))
    assert out.shape == (0, 8, 7, 7)
    out.sum().backward()
    assert x.grad is not None and (x.grad == 0).all()


# ------------------------------------------------------------------------------------------------------- clustering
def _device_tables(cuda, boxes, prev, labels, probs):
    """Per-image inputs (lists of numpy arrays) -> the device's tables as numpy, one pcl_cluster call."""
    counts = [len(b) for b in boxes]
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=cuda)
    t = pcl_cluster(torch.from_numpy(np.concatenate(boxes)).to(cuda), off, max(counts),
                    torch.from_numpy(np.concatenate(prev)).to(cuda), torch.from_numpy(np.stack(labels)).to(cuda),
                    torch.from_numpy(np.concatenate(probs)).to(cuda))
    return {k: v.cpu().numpy() for k, v in t.items()}, counts


def _check_tables(t, counts, i, want, what):
    lo, hi = sum(counts[:i]), sum(counts[:i + 1])
    G = len(want["pc_labels"])
    assert t["pc_num"][i] == G, what
    np.testing.assert_array_equal(t["row_label"][lo:hi], want["labels"], err_msg=what)
    np.testing.assert_array_equal(t["row_assign"][lo:hi], want["gt_assignment"], err_msg=what)
    np.testing.assert_array_equal(t["pc_int"][i, :G, 0], want["pc_labels"], err_msg=what)
    np.testing.assert_array_equal(t["pc_int"][i, :G, 1], want["pc_count"], err_msg=what)
    np.testing.assert_array_equal(t["pc_int"][i, :G, 2], want["centre_rows"], err_msg=what)
    assert (t["pc_int"][i, G:] == 0).all() and (t["pc_flt"][i, G:] == 0).all(), what
    np.testing.assert_allclose(t["row_weight"][lo:hi], want["cls_loss_weights"], rtol=1e-6, atol=0, err_msg=what)
    np.testing.assert_allclose(t["pc_flt"][i, :G, 0], want["centre_scores"], rtol=1e-6, atol=0, err_msg=what)
    np.testing.assert_allclose(t["pc_flt"][i, :G, 1], want["img_cls_loss_weights"], rtol=1e-6, atol=0, err_msg=what)
    np.testing.assert_allclose(t["pc_flt"][i, :G, 2], want["pc_probs"], rtol=1e-6, atol=0, err_msg=what)


@pytest.mark.parametrize("with_background", [False, True], ids=["prev-K", "prev-K+1"])
def test_clustering_matches_restatement_on_the_golden_inputs(cuda, with_background):
    cases = load_cases("pcl_reference_cases.npz")
    K = 10
    names = sorted(n for n, c in cases.items() if (c["cls_prob"].shape[1] == K + 1) == with_background)
    assert len(names) >= 6
    boxes = [cases[n]["boxes"] for n in names]
    prev = [cases[n]["cls_prob"] for n in names]
    labels = [cases[n]["im_labels"].reshape(-1) for n in names]
    probs = [cases[n]["cls_prob_new"] for n in names]
    t, counts = _device_tables(cuda, boxes, prev, labels, probs)
    for i, n in enumerate(names):
        _check_tables(t, counts, i, pcl_ref.pcl(boxes[i], prev[i], labels[i], probs[i]), n)
    again, _ = _device_tables(cuda, boxes, prev, labels, probs)
    for k in t:
        np.testing.assert_array_equal(again[k], t[k], err_msg=k)


def _synthetic_image(rng, R, K, present):
    """Proposals piled on a few objects, a previous score that favours one object's proposals per class."""
    n_obj = len(present) + 1
    ctr = rng.uniform(0.2, 0.8, (n_obj, 2)) * [500, 375]
    size = rng.uniform(60, 200, (n_obj, 2))
    which = rng.integers(0, n_obj, R)
    c = ctr[which] + rng.normal(0, 14, (R, 2))
    wh = size[which] * rng.uniform(0.6, 1.4, (R, 2))
    boxes = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, [500, 375, 500, 375]).astype(np.float32)
    z = rng.normal(0, 1, (R, K + 1))
    for k, cls in enumerate(present):
        z[which == k, cls + 1] += rng.uniform(1, 4)
    labels = np.zeros(K, np.float32)
    labels[present] = 1
    return boxes, z.astype(np.float32), labels


@pytest.mark.parametrize("counts,K", [([700, 1, 2500, 64], 20), ([3, 2], 4), ([4100], 20)],
                         ids=["ragged-20", "tiny-4", "large-20"])
def test_clustering_on_the_devices_own_probabilities(cuda, counts, K):
    """Both probability tables come from the device's soft-max; the restatement reads the same bits.  Image 1 of the
    ragged case has one proposal; the tiny case has fewer proposals than clusters could hold."""
    rng = np.random.default_rng(len(counts) * 1000 + K)
    imgs = [_synthetic_image(rng, R, K, np.sort(rng.choice(K, int(rng.integers(1, min(K, 4) + 1)), replace=False)))
            for R in counts]
    zprev = np.concatenate([im[1] for im in imgs])
    znew = rng.normal(0, 1.5, zprev.shape).astype(np.float32)
    prev = pcl_softmax(torch.from_numpy(zprev).to(cuda)).cpu().numpy()
    new = pcl_softmax(torch.from_numpy(znew).to(cuda)).cpu().numpy()
    np.testing.assert_allclose(prev, pcl_ref.softmax(zprev), rtol=1e-5, atol=1e-8)
    sp = np.cumsum(counts)[:-1]
    boxes, labels = [im[0] for im in imgs], [im[2] for im in imgs]
    t, _ = _device_tables(cuda, boxes, np.split(prev, sp), labels, np.split(new, sp))
    for i in range(len(counts)):
        _check_tables(t, counts, i, pcl_ref.pcl(boxes[i], np.split(prev, sp)[i], labels[i], np.split(new, sp)[i]),
                      "image %d" % i)
    again, _ = _device_tables(cuda, boxes, np.split(prev, sp), labels, np.split(new, sp))
    for k in t:
        np.testing.assert_array_equal(again[k], t[k], err_msg=k)


def test_image_without_a_present_class_is_all_background(cuda):
    rng = np.random.default_rng(4)
    boxes, z, labels = _synthetic_image(rng, 50, 5, np.array([1]))
    p = pcl_ref.softmax(z).astype(np.float32)
    t, _ = _device_tables(cuda, [boxes], [p], [np.zeros(5, np.float32)], [p])
    assert t["pc_num"][0] == 0 and (t["row_label"] == 0).all() and (t["row_assign"] == -1).all()
    assert (t["row_weight"] == 0).all()


# ------------------------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("counts", [[900, 300], [64], [5, 2000, 40]])
def test_pcl_loss_and_logit_gradient_against_fp64(cuda, counts):
    K = 20
    rng = np.random.default_rng(sum(counts))
    imgs = [_synthetic_image(rng, R, K, np.sort(rng.choice(K, 2, replace=False))) for R in counts]
    boxes, labels = [im[0] for im in imgs], [im[2] for im in imgs]
    prev = [pcl_ref.softmax(im[1]).astype(np.float32) for im in imgs]
    wide = (rng.normal(0, 2, (sum(counts), K + 1 + 7))).astype(np.float32)     # the logits are columns of a wider matrix
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=cuda)
    wd = torch.from_numpy(wide).to(cuda).requires_grad_()
    loss, probs, t = pcl_loss(wd[:, 3:3 + K + 1], torch.from_numpy(np.concatenate(boxes)).to(cuda), off, max(counts),
                              torch.from_numpy(np.concatenate(prev)).to(cuda), torch.from_numpy(np.stack(labels)).to(cuda))
    (loss * 1.7).backward()
    assert not probs.requires_grad
    # fp64 evaluation of the same formula on the tables the restatement derives from the device's probabilities
    sp = np.cumsum(counts)[:-1]
    z = wide[:, 3:3 + K + 1].astype(np.float64)
    pd = probs.cpu().numpy()
    want_loss, want_grad = 0.0, []
    for i, (zi, pi) in enumerate(zip(np.split(z, sp), np.split(pd, sp))):
        ti = pcl_ref.pcl(boxes[i], prev[i], labels[i], pi)
        # pc_prob from the fp64 probabilities, as the formula has it
        p64 = pcl_ref.softmax(zi)
        for j in range(len(ti["pc_labels"])):
            m = ti["gt_assignment"] == j
            if m.any():
                ti["pc_probs"][j] = np.clip(p64[m, ti["pc_labels"][j]], 1e-9, 1 - 1e-9).mean()
        want_loss += pcl_ref.loss(p64, ti) / len(counts)
        want_grad.append(pcl_ref.loss_grad_logits(zi, ti, upstream=1.7, images=len(counts)))
    rel_close(loss, torch.tensor(want_loss), what="loss")
    g = wd.grad.cpu()
    rel_close(g[:, 3:3 + K + 1], torch.from_numpy(np.concatenate(want_grad)), what="d logits")
    assert g[:, :3].abs().max() == 0 and g[:, 3 + K + 1:].abs().max() == 0


def test_pcl_branch_reads_nothing_back_to_the_host(cuda, monkeypatch):
    """Between the logits and the loss, and through the backward, no .cpu() / .item() / .tolist() / .numpy() runs
    and the runtime sees no synchronising call (torch's sync debug mode raises on one)."""
    from jtsm_amd.modeling.box_regression import Box2BoxTransform
    from jtsm_amd.modeling.roi_heads.fast_rcnn_oicr import OICROutputLayers
    from jtsm_amd.structures import Instances

    K, counts = 20, [400, 250]
    rng = np.random.default_rng(2)
    imgs = [_synthetic_image(rng, R, K, np.array([3, 11])) for R in counts]
    heads = [OICROutputLayers(32, num_classes=K, box2box_transform=Box2BoxTransform(weights=(10.0, 10.0, 5.0, 5.0)),
                              refine_k=k, refine_reg=[False] * 3).to(cuda) for k in range(3)]
    proposals = []
    for im in imgs:
        inst = Instances((375, 500))
        inst.proposal_boxes = Boxes(torch.from_numpy(im[0]).to(cuda))
        proposals.append(inst)
    x = torch.randn(sum(counts), 32, device=cuda)
    mil = torch.from_numpy(np.concatenate([pcl_ref.softmax(im[1])[:, 1:] / len(im[1]) for im in imgs])).float().to(cuda)
    oh = torch.from_numpy(np.stack([im[2] for im in imgs])).to(cuda)
    off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=cuda)
    predictions = [h(x) for h in heads]
    # warm-up outside the watch: the first call loads the code objects
    heads[0].losses_pcl(predictions[0], proposals, mil, oh, offsets=off)
    torch.cuda.synchronize()
    calls = []
    for name in ("cpu", "item", "tolist", "numpy"):
        orig = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _o=orig, _n=name, **k: (calls.append(_n), _o(self, *a, **k))[1])
    torch.cuda.set_sync_debug_mode("error")
    try:
        prev, losses = mil, {}
        for h, pred in zip(heads, predictions):
            losses.update(h.losses_pcl(pred, proposals, prev, oh, offsets=off))
            prev = h.pcl_probs
        sum(losses.values()).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert calls == []
    monkeypatch.undo()
    assert sorted(losses) == ["loss_cls_r0", "loss_cls_r1", "loss_cls_r2"]
    assert all(torch.isfinite(v) and float(v) > 0 for v in losses.values())
    assert all(h.cls_score.weight.grad is not None and h.cls_score.weight.grad.abs().sum() > 0 for h in heads)
