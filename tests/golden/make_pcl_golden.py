"""Records tests/golden/pcl_reference_cases.npz — build container only (it runs the reference's own
projects/WSL/wsl/modeling/roi_heads/third_party/pcl.py with scikit-learn, where it lies; nothing of it is copied).

    python tests/golden/make_pcl_golden.py

The reference module imports detectron2.structures for Boxes / pairwise_iou; this repository's implementations of the
two stand in.  Per case the file holds the inputs (boxes, cls_prob, im_labels, cls_prob_new), the top-ranking sets
scikit-learn's KMeans returned (pool-relative indices per present class: top_flat / top_len) and the reference's eight
output arrays.  Only seeds for which the restatement (tests/pcl_ref.py, fed the recorded sets) meets no degree tie, no
score tie and no duplicate box are kept — there the reference's result does not hang on its unstable argsort — and
seeds are tried until 24 cases are kept."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
REF = "/root/reference/projects/WSL/wsl/modeling/roi_heads/third_party/pcl.py"
OUT = os.path.join(HERE, "pcl_reference_cases.npz")
CASES, K = 24, 10
FIELDS = ("labels", "cls_loss_weights", "gt_assignment", "pc_labels", "pc_probs", "pc_count", "img_cls_loss_weights",
          "im_labels_real")


def reference_module():
    from jtsm_amd.structures import Boxes, pairwise_iou

    d2 = types.ModuleType("detectron2")
    st = types.ModuleType("detectron2.structures")
    st.Boxes = lambda a: Boxes(torch.as_tensor(np.asarray(a, np.float32).reshape(-1, 4)))
    st.pairwise_iou = pairwise_iou
    d2.structures = st
    sys.modules.setdefault("detectron2", d2)
    sys.modules.setdefault("detectron2.structures", st)
    spec = importlib.util.spec_from_file_location("reference_pcl", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_inputs(seed):
    """A few hundred proposals piled on a few objects; 1-4 present classes; the previous scores favour the proposals
    near an object of the class; with or without a background column in front."""
    rng = np.random.default_rng(seed)
    R = int(rng.integers(200, 400))
    n_present = int(rng.integers(1, 5))
    present = np.sort(rng.choice(K, n_present, replace=False))
    W, H = 500.0, 375.0
    ctr = rng.uniform(0.2, 0.8, (n_present + 1, 2)) * [W, H]
    size = rng.uniform(60, 200, (n_present + 1, 2))
    which = rng.integers(0, n_present + 1, R)
    c = ctr[which] + rng.normal(0, 12, (R, 2))
    wh = size[which] * rng.uniform(0.6, 1.4, (R, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1)
    boxes = np.clip(boxes, 0, [W, H, W, H]).astype(np.float32)
    logits = rng.normal(0, 1, (R, K + 1))
    for k, cls in enumerate(present):               # a handful of high scorers per class among the object's proposals
        near = np.nonzero(which == k)[0]
        hi = rng.choice(near, min(len(near), int(rng.integers(4, 30))), replace=False)
        logits[near, cls + 1] += rng.uniform(0.5, 1.5)
        logits[hi, cls + 1] += rng.uniform(3, 5)
    e = np.exp(logits - logits.max(1, keepdims=True))
    prev = (e / e.sum(1, keepdims=True)).astype(np.float32)
    if seed % 2:                                    # the first branch: MIL scores, no background column
        prev = (prev[:, 1:] / R).astype(np.float32)
    z = rng.normal(0, 1.5, (R, K + 1))
    e = np.exp(z - z.max(1, keepdims=True))
    new = (e / e.sum(1, keepdims=True)).astype(np.float32)
    labels = np.zeros((1, K), np.float32)
    labels[0, present] = 1
    return boxes, prev, labels, new


def main():
    import pcl_ref

    mod = reference_module()
    kept, seed, out = 0, 0, {}
    while kept < CASES:
        seed += 1
        boxes, prev, labels, new = make_inputs(seed)
        sets = []
        inner = mod._get_top_ranking_propoals

        def recording(probs, inner=inner, sets=sets):
            idx = inner(probs)
            sets.append(np.asarray(idx).copy())
            return idx

        mod._get_top_ranking_propoals = recording
        try:
            want = mod.PCL(boxes.copy(), torch.from_numpy(prev.copy()), labels.copy(), torch.from_numpy(new.copy()))
        finally:
            mod._get_top_ranking_propoals = inner
        try:
            info = pcl_ref.pcl(boxes, prev, labels, new, top_sets=sets)["info"]
        except IndexError:                          # (a tie changed the number of centres: the pools part)
            continue
        if info["degree_tie"] or info["score_tie"] or info["duplicate_box"]:
            continue
        name = "case%02d" % kept
        out[name + "__boxes"], out[name + "__cls_prob"] = boxes, prev
        out[name + "__im_labels"], out[name + "__cls_prob_new"] = labels, new
        out[name + "__top_flat"] = np.concatenate(sets).astype(np.int32)
        out[name + "__top_len"] = np.array([len(s) for s in sets], np.int32)
        for f in FIELDS:
            out[name + "__" + f] = want[f]
        kept += 1
    np.savez_compressed(OUT, **out)
    print("kept %d cases of %d seeds -> %s (%d bytes)" % (kept, seed, OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
