"""Records tests/golden/retinanet_reference_cases.npz — in the build container only, where the reference tree exists.

    python tests/golden/make_retinanet_golden.py [/root/reference]

The reference's detectron2/modeling/matcher.py, structures/boxes.py and modeling/box_regression.py are loaded BY FILE
PATH, behind two stub modules of this file's own (detectron2.layers.nonzero_tuple, detectron2.utils.env.TORCH_VERSION),
and run on the CPU on inputs that tests/retinanet_ref.py regenerates from a seed; nothing of the reference is copied.
fvcore is not part of the reference tree: the focal and smooth-L1 formulas are restated from the reference's call
(tests/retinanet_ref.py), in fp32 torch and in fp64.  Stored — seeds and results only:

  label cases   seed, and the reference's labels (N, R) / matched indices (N, R)
  loss cases    seed, the fp64 sums of the two losses and the number of positives
  cand cases    seed, and per image the (level, anchor, class) sequence, the fp32 scores, the reference's apply_deltas
                boxes, and the positions kept by the per-class NMS and the top-100 cut
  meta          T_loss  = max relative |fp32 restatement - fp64| over the loss cases;  loss_bar  = max(1e-6, 4 T_loss)
                T_grad  = likewise on the gradients, relative to the case's largest |gradient|; grad_bar = max(1e-6, 4 T_grad)
                T_box   = max |reference fp32 apply_deltas - fp64| relative to the box's longer side; box_bar = max(1e-6, 4 T_box)
                T_score = max |fp32 sigmoid - fp64|;                                   score_bar = max(2^-23, 4 T_score)
                (the factor 4: the head-room the keypoint and rotated goldens give a kernel that sums in another order
                than the host)"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import retinanet_ref as RR  # noqa: E402

LABEL_SEEDS = {"g0": 1, "g1": 2, "g300": 3, "dup": 4, "lowq": 5, "band": 6, "zero": 7, "n3": 8}
LOSS_SEEDS = {name: 20 + i for i, name in enumerate(RR.LOSS_CASES)}
CAND_SEEDS = {"c80": 40, "c1": 50}
# which label kinds a case is there for: p positive, b background, i ignored, q a positive whose best IoU is below the
# lowest threshold (a low-quality match)
LABEL_KINDS = {"g0": "b", "g1": "pb", "g300": "pbi", "dup": "pb", "lowq": "qb", "band": "pbi", "zero": "p", "n3": "pbi"}


def load_reference(root):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    def nonzero_tuple(x):
        return x.nonzero().unbind(1)

    stub("detectron2")
    stub("detectron2.layers", nonzero_tuple=nonzero_tuple)
    stub("detectron2.utils")
    stub("detectron2.utils.env", TORCH_VERSION=tuple(int(v) for v in torch.__version__.split(".")[:2]))
    out = {}
    for name, rel in (("matcher", "modeling/matcher.py"), ("boxes", "structures/boxes.py"),
                      ("box_regression", "modeling/box_regression.py")):
        spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(root, "detectron2", rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["ref_" + name] = mod
        spec.loader.exec_module(mod)
        out[name] = mod
    return out


def reference_labels(ref, anchors, images):
    """label_anchors (meta_arch/retinanet.py:353-397) around the reference's pairwise_iou and Matcher."""
    matcher = ref["matcher"].Matcher([0.4, 0.5], [0, -1, 1], allow_low_quality_matches=True)
    boxes_cls = ref["boxes"].Boxes
    labels, matched, best = [], [], []
    for gt, cls in images:
        q = ref["boxes"].pairwise_iou(boxes_cls(torch.from_numpy(gt)), boxes_cls(torch.from_numpy(anchors)))
        idx, lab = matcher(q)
        if gt.shape[0]:
            out = torch.from_numpy(cls)[idx]
            out[lab == 0] = RR.NUM_CLASSES
            out[lab == -1] = -1
            best.append(q.max(0).values.numpy())
        else:
            out = torch.zeros_like(idx) + RR.NUM_CLASSES
            best.append(np.zeros(anchors.shape[0], np.float32))
        labels.append(out.numpy())
        matched.append(idx.numpy())
    return np.stack(labels), np.stack(matched), np.stack(best)


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    ref = load_reference(root)
    torch.set_num_threads(8)
    out = {}

    for name, seed in LABEL_SEEDS.items():
        anchors, images = RR.label_inputs(name, seed)
        labels, matched, best = reference_labels(ref, anchors, images)
        mine = [RR.label_anchors(anchors, g, c, RR.NUM_CLASSES) for g, c in images]
        assert np.array_equal(np.stack([m[0] for m in mine]), labels), name
        assert np.array_equal(np.stack([m[1] for m in mine]), matched), name
        pos = (labels >= 0) & (labels < RR.NUM_CLASSES)
        have = {"p": pos.any(), "b": (labels == RR.NUM_CLASSES).any(), "i": (labels == -1).any(),
                "q": (pos & (best < np.float32(0.4))).any()}
        for kind in LABEL_KINDS[name]:
            assert have[kind], (name, kind)
        if name == "dup":       # the anchors matched to the repeated box all name its first copy
            assert (matched == 2).sum() == 0 and (matched == 0).sum() > 0
        if name == "zero":      # every anchor's IoU with the zero-area gt is 0, that gt's maximum: all turn positive
            assert (best == 0).any() and pos.all()
        print("%s seed %d: %d anchors, %d positive, %d background, %d ignored, %d low-quality" % (
            name, seed, labels.size, int(pos.sum()), int((labels == RR.NUM_CLASSES).sum()), int((labels == -1).sum()),
            int((pos & (best < np.float32(0.4))).sum())))
        out.update({"label__%s__seed" % name: np.int64(seed), "label__%s__labels" % name: labels.astype(np.int32),
                    "label__%s__matched" % name: matched.astype(np.int32)})

    t_loss = t_grad = 0.0
    for name, seed in LOSS_SEEDS.items():
        k, _, _, alpha, gamma, beta, weights = RR.LOSS_CASES[name]
        inp = RR.loss_inputs(name, seed)
        # the targets of the positives are the reference's own get_deltas
        theirs = ref["box_regression"].Box2BoxTransform(weights=tuple(weights)).get_deltas(
            torch.from_numpy(inp["anchors"]), torch.from_numpy(inp["matched_boxes"][0])).numpy()
        mine = RR.get_deltas(inp["anchors"], inp["matched_boxes"][0], weights)
        assert np.array_equal(theirs[:, :2], mine[:, :2]), name            # (dw, dh: torch's and NumPy's fp32 log
        assert np.allclose(theirs[:, 2:], mine[:, 2:], rtol=1e-6, atol=1e-6), name   # differ in the last place)
        args = (inp["logits"], inp["deltas"], inp["labels"], inp["matched_boxes"], inp["anchors"], k, alpha, gamma, beta,
                weights)
        hi, lo = RR.losses(*args, dtype=torch.float64), RR.losses(*args, dtype=torch.float32)
        for key in ("cls", "box"):
            if hi[key]:
                t_loss = max(t_loss, abs(lo[key] - hi[key]) / abs(hi[key]))
        for key in ("d_logits", "d_deltas"):
            scale = max(float(np.abs(g).max()) for g in hi[key])
            if scale:
                t_grad = max(t_grad, max(float(np.abs(a - b).max()) for a, b in zip(lo[key], hi[key])) / scale)
        print("%s seed %d: cls %.9g box %.9g, %d positives" % (name, seed, hi["cls"], hi["box"], hi["num_pos"]))
        out.update({"loss__%s__seed" % name: np.int64(seed), "loss__%s__cls" % name: np.float64(hi["cls"]),
                    "loss__%s__box" % name: np.float64(hi["box"]), "loss__%s__num_pos" % name: np.int64(hi["num_pos"])})

    # T_box and T_score over the candidate inputs at their first seeds (the bars must not depend on the seed search)
    t_box = t_score = 0.0
    transform = ref["box_regression"].Box2BoxTransform(weights=(1.0, 1.0, 1.0, 1.0))
    for name, seed in CAND_SEEDS.items():
        inp = RR.cand_inputs(name, seed)
        for anc, x, d in zip(inp["anchors"], inp["logits"], inp["deltas"]):
            for i in range(x.shape[0]):
                b32 = transform.apply_deltas(torch.from_numpy(d[i]), torch.from_numpy(anc)).numpy()
                b64 = RR.apply_deltas(d[i], anc, (1.0, 1.0, 1.0, 1.0), np.float64)
                side = np.maximum(b64[:, 2] - b64[:, 0], b64[:, 3] - b64[:, 1])
                t_box = max(t_box, float((np.abs(b32 - b64).max(1) / side).max()))
                t_score = max(t_score, float(np.abs(RR.sigmoid32(x[i]) - 1.0 / (1.0 + np.exp(-x[i].astype(np.float64)))).max()))
    bars = {"loss_bar": max(1e-6, 4 * t_loss), "grad_bar": max(1e-6, 4 * t_grad), "box_bar": max(1e-6, 4 * t_box),
            "score_bar": max(2.0 ** -23, 4 * t_score)}
    out.update({"meta__T_loss": np.float64(t_loss), "meta__T_grad": np.float64(t_grad), "meta__T_box": np.float64(t_box),
                "meta__T_score": np.float64(t_score)})
    out.update({"meta__" + k: np.float64(v) for k, v in bars.items()})
    print("T_loss %.3g T_grad %.3g T_box %.3g T_score %.3g -> %s" % (t_loss, t_grad, t_box, t_score, bars))

    for name, seed0 in CAND_SEEDS.items():
        k, _, _, topk, above = RR.CAND_CASES[name]
        for seed in range(seed0, seed0 + 4):
            inp = RR.cand_inputs(name, seed)
            clear, per_image = True, []
            for i in range(inp["logits"][0].shape[0]):
                # unambiguous: strictly distinct fp32 scores above the threshold, gaps and the distance to the threshold
                # above score_bar (distinct scores keep the cut clear of its neighbour too)
                for x in inp["logits"]:
                    s = np.sort(RR.sigmoid32(x[i]).ravel().astype(np.float64))
                    s = s[s > 0.03]
                    assert s.size == 0 or (np.diff(s).min() > bars["score_bar"] if s.size > 1 else True), name
                    assert s.size == 0 or np.abs(s - RR.CAND_THRESH).min() > bars["score_bar"], name
                seq, scores, boxes = RR.candidates(inp, i, RR.CAND_THRESH, topk)
                kept, closest = RR.nms_per_class(boxes, scores, seq[:, 2], RR.CAND_NMS)
                clear = clear and closest > 1e-4
                per_image.append((seq, scores, boxes, kept[:RR.CAND_DETS]))
            if clear:
                break
        else:
            raise SystemExit("%s: a same-class pair within 1e-4 of the NMS threshold at every seed" % name)
        out["cand__%s__seed" % name] = np.int64(seed)
        for i, (seq, scores, boxes, kept) in enumerate(per_image):
            want = [min(topk, m) for m in above]
            assert [int((seq[:, 0] == l).sum()) for l in range(len(above))] == want, name
            # the reference's decode of the selected rows
            theirs = np.concatenate([transform.apply_deltas(
                torch.from_numpy(inp["deltas"][l][i][seq[seq[:, 0] == l, 1]]),
                torch.from_numpy(inp["anchors"][l][seq[seq[:, 0] == l, 1]])).numpy() for l in range(len(above))])
            assert float(np.abs(theirs - boxes).max()) <= bars["box_bar"] * float(np.abs(theirs).max()), name
            print("%s seed %d image %d: %d candidates, %d kept" % (name, seed, i, len(seq), len(kept)))
            out.update({"cand__%s__%d__seq" % (name, i): seq.astype(np.int32), "cand__%s__%d__scores" % (name, i): scores,
                        "cand__%s__%d__boxes" % (name, i): theirs.astype(np.float32),
                        "cand__%s__%d__kept" % (name, i): kept.astype(np.int32)})

    path = os.path.join(HERE, "retinanet_reference_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
