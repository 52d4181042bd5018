"""The host restatement of RetinaNet's device-side steps (tests/retinanet_ref.py) reproduces every vector recorded from
the reference (tests/golden/retinanet_reference_cases.npz), and the conditions the recording promises hold: the bars'
formulas, distinct candidate scores with gaps above score_bar, the label kinds each label case is there for."""
import numpy as np
import pytest
import torch

import retinanet_ref as RR

G = RR.golden()
LABEL_NAMES = sorted(RR.LABEL_CASES)
LOSS_NAMES = sorted(RR.LOSS_CASES)
CAND_NAMES = sorted(RR.CAND_CASES)


def test_bars_follow_their_formulas():
    assert G["meta__loss_bar"] == max(1e-6, 4 * G["meta__T_loss"])
    assert G["meta__grad_bar"] == max(1e-6, 4 * G["meta__T_grad"])
    assert G["meta__box_bar"] == max(1e-6, 4 * G["meta__T_box"])
    assert G["meta__score_bar"] == max(2.0 ** -23, 4 * G["meta__T_score"])
    assert G["meta__loss_bar"] < 1e-5 and G["meta__grad_bar"] < 1e-4 and G["meta__box_bar"] < 1e-5 and G["meta__score_bar"] < 1e-6


@pytest.mark.parametrize("name", LABEL_NAMES)
def test_labels(name):
    anchors, images = RR.label_inputs(name, int(G["label__%s__seed" % name]))
    assert anchors.shape[0] == 477
    want_l, want_m = G["label__%s__labels" % name], G["label__%s__matched" % name]
    for i, (gt, cls) in enumerate(images):
        labels, matched = RR.label_anchors(anchors, gt, cls, RR.NUM_CLASSES)
        assert np.array_equal(labels, want_l[i]) and np.array_equal(matched, want_m[i])


def test_label_cases_hold_what_they_are_there_for():
    k = RR.NUM_CLASSES
    lab = {n: G["label__%s__labels" % n] for n in LABEL_NAMES}
    assert (lab["g0"] == k).all()
    assert (lab["zero"] >= 0).all() and (lab["zero"] < k).all()              # the zero-area gt turns everything positive
    for n in ("g300", "band", "n3"):
        assert (lab[n] == -1).any() and (lab[n] == k).any() and ((lab[n] >= 0) & (lab[n] < k)).any()
    assert (lab["n3"][1] == k).all() and lab["n3"].shape == (3, 477)
    assert RR.label_inputs("g300", int(G["label__g300__seed"]))[1][0][0].shape[0] == 300     # more than one LDS chunk
    # the repeated box: its first copy is the arg-max, never the third row
    m = G["label__dup__matched"]
    assert (m == 0).any() and not (m == 2).any()
    # the low-quality match: positives although no IoU reaches 0.4
    anchors, images = RR.label_inputs("lowq", int(G["label__lowq__seed"]))
    best = RR.pairwise_iou(images[0][0], anchors).max(0)
    assert best.max() < 0.4 and ((lab["lowq"][0] >= 0) & (lab["lowq"][0] < k)).any()


@pytest.mark.parametrize("name", LOSS_NAMES)
def test_losses(name):
    k, _, kind, alpha, gamma, beta, weights = RR.LOSS_CASES[name]
    inp = RR.loss_inputs(name, int(G["loss__%s__seed" % name]))
    out = RR.losses(inp["logits"], inp["deltas"], inp["labels"], inp["matched_boxes"], inp["anchors"], k, alpha, gamma,
                    beta, weights)
    assert out["cls"] == float(G["loss__%s__cls" % name]) and out["box"] == float(G["loss__%s__box" % name])
    assert out["num_pos"] == int(G["loss__%s__num_pos" % name])
    flat = np.concatenate([x.ravel() for x in inp["logits"]])
    assert (flat == 50).any() and (flat == -50).any() and (flat == 0).any()
    assert {"ignored": out["cls"] == 0, "nopos": out["num_pos"] == 0 and out["cls"] > 0,
            "allpos": out["num_pos"] == inp["labels"].size, "mixed": 0 < out["num_pos"] < inp["labels"].size}[kind]
    assert all(a.shape[1] % 64 for a in inp["logits"])        # HWA of a level: no multiple of a wavefront, let alone a workgroup


def test_focal_gradient_closed_form():
    """The derivative the kernel uses, against autograd in fp64."""
    x = torch.linspace(-30, 30, 241, dtype=torch.float64)
    for t in (0.0, 1.0):
        for alpha, gamma in ((0.25, 2.0), (0.25, 0.0), (-1.0, 1.5)):
            xi = x.clone().requires_grad_()
            RR.focal_sum(xi, torch.full_like(x, t), alpha, gamma).backward()
            p = torch.sigmoid(x)
            ce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
            q = (1 - p) if t else p
            dq = -(p * (1 - p)) if t else p * (1 - p)
            at = 1.0 if alpha < 0 else (alpha if t else 1 - alpha)
            mine = at * ((p - t) * q ** gamma + ce * (gamma * q ** (gamma - 1) if gamma else 0.0) * dq)
            assert float((mine - xi.grad).abs().max()) < 1e-12


def test_ema():
    v = 100.0
    for n in (7, 0, 300):
        v = RR.ema(v, n)
    assert v == 0.9 * (0.9 * (0.9 * 100.0 + (1 - 0.9) * 7) + (1 - 0.9) * 1) + (1 - 0.9) * 300


@pytest.mark.parametrize("name", CAND_NAMES)
def test_candidates(name):
    k, _, maps, topk, above = RR.CAND_CASES[name]
    inp = RR.cand_inputs(name, int(G["cand__%s__seed" % name]))
    bar, box_bar = float(G["meta__score_bar"]), float(G["meta__box_bar"])
    for i in range(2):
        seq, scores, boxes = RR.candidates(inp, i, RR.CAND_THRESH, topk)
        assert np.array_equal(seq, G["cand__%s__%d__seq" % (name, i)])
        assert np.array_equal(scores, G["cand__%s__%d__scores" % (name, i)])
        want = G["cand__%s__%d__boxes" % (name, i)]
        side = np.maximum(want[:, 2] - want[:, 0], want[:, 3] - want[:, 1])
        assert float((np.abs(boxes - want).max(1) / side).max()) <= box_bar
        kept, closest = RR.nms_per_class(boxes, scores, seq[:, 2], RR.CAND_NMS)
        assert closest > 1e-4 and np.array_equal(kept[:RR.CAND_DETS], G["cand__%s__%d__kept" % (name, i)])
        assert [int((seq[:, 0] == l).sum()) for l in range(len(maps))] == [min(topk, m) for m in above]
        for x in inp["logits"]:          # the recorded promise: distinct scores, clear of each other and the threshold
            s = np.sort(RR.sigmoid32(x[i]).ravel().astype(np.float64))
            s = s[s > 0.03]
            assert s.size == 0 or np.abs(s - RR.CAND_THRESH).min() > bar
            assert s.size < 2 or np.diff(s).min() > bar
            assert float(x[i][RR.sigmoid32(x[i]) <= 0.03].max()) <= -4.0
    assert above[0] > topk and 0 < above[1] < topk and (name != "c80" or above[2] == 0)


def test_tie_rule_and_unbounded_threshold():
    x = np.full((6, 4), 20.0, np.float32)            # saturated: one fp32 score
    idx, s = RR.select_level(x, 0.05, 5)
    assert list(idx) == [0, 1, 2, 3, 4] and len(set(s.tolist())) == 1
    x[2, 1] = np.nan
    idx, _ = RR.select_level(x, -1e9, 100)
    assert 9 not in idx and len(idx) == 23           # a NaN never passes
