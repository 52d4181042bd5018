"""GPU suite: the RetinaNet kernels (jtsm_amd/csrc/retinanet.hip) against the vectors recorded from the reference
(tests/golden/retinanet_reference_cases.npz) and the host restatement (tests/retinanet_ref.py).

* labels: the reference's integers exactly — G = 0 / 1 / 300, a repeated gt, a low-quality match, the ignore band, a
  zero-area gt, N = 3 with an empty image in the middle; 477 anchors;
* losses: within loss_bar of fp64, gradients within grad_bar (relative to the case's largest |gradient|); maps in the
  head's layout (A rows per cell, channel padding filled with NaN: it is never read and its gradient is zero) and as
  the reference's (N, HWA, K) views, which give the same bits; the EMA over three training calls against Python
  doubles; two identical calls give identical bits;
* candidates: the (level, anchor, class) sequence identical, scores within score_bar, boxes within box_bar, and after
  the batched NMS and the top-100 cut the same detections in the same order; saturated logits order by flat index;
  score_thresh = -1e9 returns exactly topk per level out of a workspace that does not know the threshold."""
import numpy as np
import pytest
import torch

import retinanet_ref as RR

pytestmark = pytest.mark.gpu

G = RR.golden()
BAR = {k: float(G["meta__" + k]) for k in ("loss_bar", "grad_bar", "box_bar", "score_bar")}


def dev(a, cuda, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(cuda)


def as_map(x, hw, a, pad, cuda):
    """(N, HWA, K) array -> leaf (N, H, W, A * K + pad) with NaN padding, and its (N, A * K, H, W) channel slice: what
    the head's convolutions return."""
    n, hwa, k = x.shape
    h, w = hw
    buf = torch.full((n, h, w, a * k + pad), float("nan"), dtype=torch.float32)
    buf[..., :a * k] = torch.from_numpy(x).reshape(n, h, w, a * k)
    leaf = buf.to(cuda).requires_grad_()
    return leaf, leaf.permute(0, 3, 1, 2)[:, :a * k]


# ---- labels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RR.LABEL_CASES))
def test_labels(name, cuda):
    from jtsm_amd.layers.retinanet import retinanet_label_anchors

    anchors, images = RR.label_inputs(name, int(G["label__%s__seed" % name]))
    boxes = np.concatenate([g for g, _ in images])
    classes = np.concatenate([c for _, c in images])
    labels, matched, offsets, num_pos = retinanet_label_anchors(
        dev(anchors, cuda), dev(boxes, cuda), dev(classes, cuda), [len(g) for g, _ in images], RR.NUM_CLASSES)
    want = G["label__%s__labels" % name]
    assert labels.dtype == torch.int32 and matched.dtype == torch.int32
    assert np.array_equal(labels.cpu().numpy(), want)
    assert np.array_equal(matched.cpu().numpy(), G["label__%s__matched" % name])
    assert int(num_pos) == int(((want >= 0) & (want < RR.NUM_CLASSES)).sum())
    assert offsets.tolist() == np.concatenate([[0], np.cumsum([len(g) for g, _ in images])]).tolist()


def test_label_table_is_not_hard_wired(cuda):
    from jtsm_amd.layers.retinanet import retinanet_label_anchors

    anchors, images = RR.label_inputs("band", int(G["label__band__seed"]))
    gt, cls = images[0]
    for thresholds, table in (((0.3, 0.7), (0, -1, 1)), ((0.5,), (0, 1)), ((0.2, 0.4, 0.6), (-1, 0, -1, 1))):
        labels, matched, _, _ = retinanet_label_anchors(dev(anchors, cuda), dev(gt, cuda), dev(cls, cuda), [len(gt)],
                                                        RR.NUM_CLASSES, thresholds, table)
        want_l, want_m = RR.label_anchors(anchors, gt, cls, RR.NUM_CLASSES, thresholds, table)
        assert np.array_equal(labels[0].cpu().numpy(), want_l) and np.array_equal(matched[0].cpu().numpy(), want_m)


# ---- losses ----------------------------------------------------------------------------------------------------------
def loss_case(name, cuda, as_views=False):
    k, pad, _, alpha, gamma, beta, weights = RR.LOSS_CASES[name]
    inp = RR.loss_inputs(name, int(G["loss__%s__seed" % name]))
    a = inp["A"]
    leaves, maps = [], ([], [])
    for which, (arrays, kk, p) in enumerate(((inp["logits"], k, pad), (inp["deltas"], 4, -(a * 4) % 8))):
        for x, hw in zip(arrays, inp["maps"]):
            if as_views:
                leaf = dev(x, cuda).requires_grad_()
                view = leaf
            else:
                leaf, view = as_map(x, hw, a, p, cuda)
            leaves.append(leaf)
            maps[which].append(view)
    gt = np.concatenate(inp["gt"])
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in inp["gt"]])])
    args = dict(labels=dev(inp["labels"], cuda, torch.int32), matched=dev(inp["matched"], cuda, torch.int32),
                anchors=dev(inp["anchors"], cuda), gt_boxes=dev(gt, cuda), gt_offsets=dev(offsets, cuda, torch.int32),
                num_classes=k, alpha=alpha, gamma=gamma, beta=beta, weights=weights)
    want = RR.losses(inp["logits"], inp["deltas"], inp["labels"], inp["matched_boxes"], inp["anchors"], k, alpha, gamma,
                     beta, weights)
    return inp, leaves, maps, args, want


def run_loss(maps, args, normalizer, num_pos, training=True):
    from jtsm_amd.layers.retinanet import retinanet_loss
    return retinanet_loss(maps[0], maps[1], args["labels"], args["matched"], args["anchors"], args["gt_boxes"],
                          args["gt_offsets"], num_pos, normalizer, args["num_classes"], alpha=args["alpha"],
                          gamma=args["gamma"], beta=args["beta"], weights=args["weights"], training=training)


@pytest.mark.parametrize("name", sorted(RR.LOSS_CASES))
def test_losses(name, cuda):
    inp, leaves, maps, args, want = loss_case(name, cuda)
    assert want["cls"] == float(G["loss__%s__cls" % name]) and want["box"] == float(G["loss__%s__box" % name])
    normalizer = torch.full((1,), 100.0, dtype=torch.float64, device=cuda)
    num_pos = torch.tensor([want["num_pos"]], dtype=torch.int32, device=cuda)
    loss_cls, loss_box = run_loss(maps, args, normalizer, num_pos)
    (loss_cls + loss_box).backward()
    torch.cuda.synchronize()
    state = RR.ema(100.0, want["num_pos"])
    assert float(normalizer) == state                                  # max(num_pos, 1) where there is no positive
    norm = float(np.float32(state))
    for got, key in ((loss_cls, "cls"), (loss_box, "box")):
        got, ref = float(got.detach()), want[key] / norm
        print(name, key, got, ref, abs(got - ref) / ref if ref else 0.0)
        assert abs(got - ref) <= BAR["loss_bar"] * abs(ref)
    levels = len(inp["maps"])
    for which, (key, kk) in enumerate((("d_logits", args["num_classes"]), ("d_deltas", 4))):
        scale = max(float(np.abs(g).max()) for g in want[key]) / norm
        for l in range(levels):
            leaf = leaves[which * levels + l]
            used = inp["A"] * kk
            got = leaf.grad[..., :used].reshape(want[key][l].shape).cpu().numpy().astype(np.float64)
            assert not bool(leaf.grad[..., used:].any())                # the padding's gradient: zeros, never NaN
            err = float(np.abs(got - want[key][l] / norm).max())
            print(name, key, l, err / scale if scale else err)
            assert err <= BAR["grad_bar"] * scale


def test_views_give_the_same_bits_and_calls_repeat(cuda):
    """The reference's (N, HWA, K) views (A = 1, row stride K) against the head's maps (A = 3, padded cells), each run
    twice without touching the normaliser."""
    out = []
    for as_views in (False, True, False, True):
        inp, leaves, maps, args, want = loss_case("k80pad", cuda, as_views)
        normalizer = torch.full((1,), 37.5, dtype=torch.float64, device=cuda)
        num_pos = torch.tensor([want["num_pos"]], dtype=torch.int32, device=cuda)
        a, b = run_loss(maps, args, normalizer, num_pos, training=False)
        (2 * a + 3 * b).backward()
        assert float(normalizer) == 37.5
        grads = [leaf.grad[..., :3 * (80 if i < 3 else 4)].reshape(2, -1) if not as_views else leaf.grad.reshape(2, -1)
                 for i, leaf in enumerate(leaves)]
        out.append([a.detach(), b.detach()] + grads)
    for other in out[1:]:
        assert all(torch.equal(x, y) for x, y in zip(out[0], other))


def test_normalizer_ema_over_three_training_calls(cuda):
    inp, leaves, maps, args, want = loss_case("k3", cuda)
    normalizer = torch.full((1,), 100.0, dtype=torch.float64, device=cuda)
    state = 100.0
    for n in (want["num_pos"], 0, 3 * want["num_pos"]):
        num_pos = torch.tensor([n], dtype=torch.int32, device=cuda)
        with torch.no_grad():
            loss_cls, _ = run_loss(maps, args, normalizer, num_pos)
        state = RR.ema(state, n)
        assert float(normalizer) == state
        ref = want["cls"] / float(np.float32(state))
        assert abs(float(loss_cls) - ref) <= BAR["loss_bar"] * ref


# ---- candidates ------------------------------------------------------------------------------------------------------
def cand_maps(inp, cuda):
    a = inp["A"]
    maps = ([], [])
    for l, anc in enumerate(inp["anchors"]):
        hw = (1, anc.shape[0] // a)                  # the selection sees cells, not the map's shape
        maps[0].append(as_map(inp["logits"][l], hw, a, 0, cuda)[1].detach())
        maps[1].append(as_map(inp["deltas"][l], hw, a, -(a * 4) % 8, cuda)[1].detach())
    return maps


@pytest.mark.parametrize("name", sorted(RR.CAND_CASES))
def test_candidates_and_detections(name, cuda):
    from jtsm_amd.layers.postprocess import batched_nms_device
    from jtsm_amd.layers.retinanet import retinanet_candidates

    k, _, _, topk, above = RR.CAND_CASES[name]
    inp = RR.cand_inputs(name, int(G["cand__%s__seed" % name]))
    logits, deltas = cand_maps(inp, cuda)
    anchors = dev(np.concatenate(inp["anchors"]), cuda)
    boxes, scores, classes, counts, rows = retinanet_candidates(logits, deltas, anchors, k, RR.CAND_THRESH, topk,
                                                                return_rows=True)
    levels = len(above)
    assert tuple(boxes.shape) == (2, levels * topk, 4) and classes.dtype == torch.int64
    assert counts.tolist() == [[min(topk, m) for m in above]] * 2
    for i in range(2):
        seq = G["cand__%s__%d__seq" % (name, i)]
        used = (classes[i] >= 0).cpu().numpy()
        slots = np.nonzero(used)[0]
        assert np.array_equal(used.reshape(levels, topk).sum(1), counts[i].cpu().numpy())
        assert all(used.reshape(levels, topk)[l, :c].all() for l, c in enumerate(counts[i].tolist()))
        got = np.stack([slots // topk, rows[i].cpu().numpy()[slots], classes[i].cpu().numpy()[slots]], 1)
        assert np.array_equal(got, seq)
        assert float(np.abs(scores[i].cpu().numpy()[slots] - G["cand__%s__%d__scores" % (name, i)]).max()) <= BAR["score_bar"]
        want = G["cand__%s__%d__boxes" % (name, i)]
        side = np.maximum(want[:, 2] - want[:, 0], want[:, 3] - want[:, 1])
        assert float((np.abs(boxes[i].cpu().numpy()[slots] - want).max(1) / side).max()) <= BAR["box_bar"]
        assert not bool(boxes[i][~torch.from_numpy(used).to(cuda)].any())
        keep, num, ovf = batched_nms_device(boxes[i], scores[i], classes[i], RR.CAND_NMS, k, levels * topk, 2)
        assert int(ovf) == 0
        kept = keep[:int(num)][:RR.CAND_DETS].cpu().numpy()
        compact = {int(s): j for j, s in enumerate(slots)}
        assert [compact[int(s)] for s in kept] == G["cand__%s__%d__kept" % (name, i)].tolist()


def test_saturated_logits_order_by_flat_index(cuda):
    from jtsm_amd.layers.retinanet import retinanet_candidates

    k, a, topk = 20, 3, 50
    anc = RR.level_anchors(4, 5, 8, RR.SIZES[0][:1])
    x = np.full((1, anc.shape[0], k), 20.0, np.float32)
    x[0, 0, 3] = np.nan                                                   # never passes
    x[0, 1, 0] = np.inf                                                   # score 1, as 20.0 gives in fp32: no earlier place
    d = np.zeros((1, anc.shape[0], 4), np.float32)
    logits = [as_map(x, (4, 5), a, 0, cuda)[1].detach()]
    deltas = [as_map(d, (4, 5), a, 4, cuda)[1].detach()]
    boxes, scores, classes, counts, rows = retinanet_candidates(logits, deltas, dev(anc, cuda), k, 0.05, topk,
                                                                return_rows=True)
    idx, s = RR.select_level(x[0], 0.05, topk)
    assert list(idx) == [i for i in range(topk + 1) if i != 3] and len(set(s.tolist())) == 1
    assert counts.tolist() == [[topk]]
    assert np.array_equal(rows[0].cpu().numpy() * k + classes[0].cpu().numpy(), idx)
    assert float(np.abs(scores[0].cpu().numpy() - s).max()) <= BAR["score_bar"]
    assert np.array_equal(boxes[0].cpu().numpy(), anc[idx // k])          # zero deltas decode to the anchors


def test_unbounded_threshold_returns_topk_from_a_fixed_workspace(cuda):
    from jtsm_amd.layers.retinanet import retinanet_candidates, retinanet_candidates_workspace_bytes

    k, a, topk = 80, 9, 1000
    maps = [(16, 16), (8, 8), (4, 4)]
    rs = np.random.RandomState(5)
    anchors = RR.pyramid_anchors(maps)
    xs = [(rs.randn(2, anc.shape[0], k) * 2).astype(np.float32) for anc in anchors]
    ds = [(rs.randn(2, anc.shape[0], 4) * 0.3).astype(np.float32) for anc in anchors]
    logits = [as_map(x, hw, a, 0, cuda)[1].detach() for x, hw in zip(xs, maps)]
    deltas = [as_map(d, hw, a, 4, cuda)[1].detach() for d, hw in zip(ds, maps)]
    flat = dev(np.concatenate(anchors), cuda)
    ws = retinanet_candidates_workspace_bytes(2, 3, topk)
    assert ws <= 2 * 3 * (65536 * 4 + topk * 8 + 256) + 4096              # histograms and topk keys: no term in the elements
    for thresh in (-1e9, 0.05):
        boxes, scores, classes, counts, rows = retinanet_candidates(logits, deltas, flat, k, thresh, topk, return_rows=True)
        assert counts.tolist() == [[topk] * 3] * 2
        for i in range(2):
            for l in range(3):
                sl = slice(l * topk, (l + 1) * topk)
                s = scores[i, sl].cpu().numpy()
                f = rows[i, sl].cpu().numpy().astype(np.int64) * k + classes[i, sl].cpu().numpy()
                idx, want = RR.select_level(xs[l][i], thresh, topk)
                assert np.all(np.diff(s) <= 0) and len(set(f.tolist())) == topk
                assert np.all((np.diff(s) < 0) | (np.diff(f) > 0))        # equal scores: lower flat index first
                assert float(np.abs(s - want).max()) <= BAR["score_bar"]
                assert float(np.abs(s - RR.sigmoid32(xs[l][i]).ravel()[f]).max()) <= BAR["score_bar"]
                # the same set but for elements within score_bar of the cut
                clear = RR.sigmoid32(xs[l][i]).ravel()[idx] > want[-1] + 2 * BAR["score_bar"]
                assert set(idx[clear].tolist()) <= set(f.tolist())
