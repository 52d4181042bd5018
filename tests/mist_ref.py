"""torch-CPU restatement of the reference's MIST pseudo-ground-truth mining, operation by operation:

    get_pgt_top_k(top_k=0.15, thres=0, need_instance=False)   projects/WSL/wsl/modeling/roi_heads/roi_heads_oicr.py:660-792
    get_pgt_mist                                               :550-591
    label_and_sample_proposals (Matcher([0.5], [0, 1]), no sub-sampling)   oracle/model.py match_and_label

The reference method itself cannot be run here: it needs detectron2 and torchvision (batched_nms), and neither is
installed.  Its NMS is oracle.inference.batched_nms, which tests/golden/nms_ref.npz pins to the reference's compiled
greedy loop.  torch.topk leaves the order of equal scores open; this restatement takes the first rows of a STABLE
descending sort (equal scores: lower row first), which is torch.topk wherever the scores differ.

Also the generator of the piled cases the GPU tests run (tests/test_hip_mist.py, tests/test_hip_oicr_model.py), with
the conditions under which the integer results are well defined, checked in float64."""
import numpy as np
import torch

from oracle import inference as OI
from oracle import model as OM


def top_t(num_pred, top_pro):
    return max(int(num_pred * top_pro), 1)                                        # :727


def candidates(boxes_per_class, scores, class_ids, top_pro=0.15):
    """get_pgt_top_k for one image.  boxes_per_class (n, K, 4), scores (n, >= K), class_ids (G,) int64.
    -> dict(scores (t*G,), boxes (t*G, 4), classes (t*G,), rows (t*G,), t): the (t, G) tensors flattened."""
    n, G = scores.shape[0], class_ids.numel()
    sc = torch.index_select(scores, 1, class_ids)                                 # :713-716
    bx = torch.index_select(boxes_per_class, 1, class_ids)                        # :717-720
    t = top_t(n, top_pro)
    order = torch.sort(sc, dim=0, descending=True, stable=True)                   # torch.topk(sc, t, dim=0), :730-733
    pgt_scores, pgt_idxs = order.values[:t], order.indices[:t]
    pgt_boxes = torch.gather(bx, 0, pgt_idxs[:, :, None].expand(t, G, 4))         # :736-743
    pgt_classes = class_ids[None, :].expand(t, G)                                 # :744-747
    return dict(scores=pgt_scores.reshape(-1), boxes=pgt_boxes.reshape(-1, 4), classes=pgt_classes.reshape(-1),
                rows=pgt_idxs.reshape(-1), t=t)                                   # :783-785


def mist(boxes_per_class, scores, class_ids, top_pro=0.15, thr=0.2):
    """get_pgt_mist for one image -> dict(boxes, classes, scores, weights, rows), survivors in NMS order."""
    if class_ids.numel() == 0:
        e = torch.zeros(0)
        return dict(boxes=torch.zeros(0, 4), classes=torch.zeros(0, dtype=torch.int64), scores=e, weights=e,
                    rows=torch.zeros(0, dtype=torch.int64))
    c = candidates(boxes_per_class, scores, class_ids, top_pro)
    keep = OI.batched_nms(c["boxes"], c["scores"], torch.zeros_like(c["classes"]), thr)      # :564-568
    return dict(boxes=c["boxes"][keep], classes=c["classes"][keep], scores=c["scores"][keep],
                weights=c["scores"][keep], rows=c["rows"][keep])                  # :569-586: gt_weights = pgt_scores


def label(prop_boxes, tgt, bg):
    """label_and_sample_proposals for one image -> dict(classes, idx[, boxes, scores, weights])."""
    return OM.match_and_label(prop_boxes, tgt, nt=bg)


def branch_inputs(mode, scores_or_logits, deltas, boxes, K):
    """(boxes_per_class (n, K, 4), scores (n, .)) as the head hands them to get_pgt_mist: `raw` — the MIL scores and
    the proposals (k = 0); `reg` / `noreg` — the previous branch's soft-max and its decoded boxes, zero deltas for a
    branch without regression (OICROutputLayers.forward)."""
    n = boxes.shape[0]
    if mode == "raw":
        return boxes[:, None, :].expand(n, K, 4), scores_or_logits
    d = deltas if mode == "reg" else torch.zeros(n, 4 * K, dtype=boxes.dtype)
    return OM.apply_deltas(d, boxes).view(n, K, 4), torch.softmax(scores_or_logits, dim=-1)


# ----------------------------------------------------------------------------------------------------------------
# piled cases
def _iou64(a, b):
    a, b = a.double(), b.double()
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(a[:, None, 2:], b[:, 2:]) - torch.max(a[:, None, :2], b[:, :2])).clamp(min=0)
    inter = wh.prod(dim=2)
    return inter / (area_a[:, None] + area_b - inter)


def make_image(rng, n, class_ids, K, jitter=0.02):
    """n proposals piled around a few rectangles — three per present class and three of no class, the first two
    overlapping at IoU about 1/3 (suppressed by one another, never matched to one another), the rest apart — with class
    probabilities (n, K + 1) (background last) taken from a geometric grid of 3e-4 steps, so that no two (row, class)
    entries of the image are closer than that; a class's own piles hold its best rows."""
    G = len(class_ids)
    piles = 3 * (G + 1)
    side = rng.uniform(70.0, 110.0, (piles, 2))
    origin = np.stack([30.0 + 260.0 * (np.arange(piles) % 5), 30.0 + 260.0 * (np.arange(piles) // 5)], 1)
    origin = origin + rng.uniform(0.0, 40.0, (piles, 2))
    if piles > 1:                                    # pile 1 sits half a side right of pile 0: IoU = 1/3 before jitter
        side[1] = side[0]
        origin[1] = origin[0] + [side[0, 0] / 2, 0.0]
    which = rng.integers(0, piles, n)
    which[:min(n, piles)] = np.arange(piles)[:min(n, piles)]
    rect = np.concatenate([origin, origin + side], 1)[which]
    wh = np.concatenate([side, side], 1)[which]
    boxes = (rect + rng.uniform(-jitter, jitter, (n, 4)) * wh).astype(np.float32)
    # probabilities: every (row, present class) pair takes its own level of the grid
    key = rng.uniform(0.0, 1.0, (n, max(G, 1))) + (which[:, None] % (G + 1) != np.arange(max(G, 1))[None, :])
    level = np.empty(n * max(G, 1), dtype=np.int64)
    level[np.argsort(key.reshape(-1), kind="stable")] = np.arange(n * max(G, 1))
    p_present = 0.12 * np.exp(-3e-4 * level.reshape(n, max(G, 1)))
    probs = np.zeros((n, K + 1))
    absent = np.setdiff1d(np.arange(K + 1), np.asarray(class_ids, dtype=np.int64))
    if G:
        probs[:, np.asarray(class_ids)] = p_present
    rest = rng.uniform(0.5, 1.5, (n, len(absent)))
    probs[:, absent] = rest / rest.sum(1, keepdims=True) * (1.0 - probs.sum(1, keepdims=True))
    return torch.from_numpy(boxes), torch.from_numpy(probs)


def make_case(seed, rows, classes_per_image, K=20, mode="raw", delta_scale=0.1):
    """One batch: dict(boxes [n_i,4], class_ids [G_i], scores (R, K) float32 for `raw` / logits (R, K+1) otherwise,
    deltas (R, 4K) for `reg`), drawn from `seed`."""
    rng = np.random.default_rng(seed)
    boxes, class_ids, tables = [], [], []
    for n, G in zip(rows, classes_per_image):
        ids = np.sort(rng.choice(K, G, replace=False))
        b, p = make_image(rng, n, ids, K)
        boxes.append(b)
        class_ids.append(torch.from_numpy(ids.astype(np.int64)))
        tables.append(p)
    probs = torch.cat(tables)
    R = probs.shape[0]
    case = dict(boxes=boxes, class_ids=class_ids, mode=mode, rows=list(rows), K=K, seed=seed, deltas=None)
    if mode == "raw":
        case["scores"] = probs[:, :K].to(torch.float32).contiguous()
    else:
        shift = torch.from_numpy(rng.uniform(-2.0, 2.0, (R, 1)))
        case["scores"] = (probs.log() + shift).to(torch.float32).contiguous()
        if mode == "reg":
            case["deltas"] = torch.from_numpy(rng.normal(0.0, delta_scale, (R, 4 * K))).to(torch.float32)
    return case


def image_inputs(case, i):
    lo = sum(case["rows"][:i])
    hi = lo + case["rows"][i]
    d = case["deltas"][lo:hi] if case["deltas"] is not None else None
    return branch_inputs(case["mode"], case["scores"][lo:hi], d, case["boxes"][i], case["K"])


def well_defined(case, top_pro=0.15):
    """The conditions under which rows, classes, num, labels and matched indices do not hang on rounding, from the
    restatement in float64: candidate scores of an image pairwise distinct (relative gap >= 1e-4 in the logits
    modes), every candidate-pair IoU >= 1e-3 away from 0.2, every proposal-survivor IoU >= 1e-4 away from 0.5."""
    for i, ids in enumerate(case["class_ids"]):
        if ids.numel() == 0 or case["rows"][i] == 0:
            continue
        bpc, sc = image_inputs(case, i)
        lo = sum(case["rows"][:i])
        if case["mode"] != "raw":
            sc = torch.softmax(case["scores"][lo:lo + case["rows"][i]].double(), dim=-1)
        c = candidates(bpc.double(), sc.double(), ids, top_pro)
        s = torch.sort(c["scores"]).values
        gap = (s[1:] - s[:-1]) / s[1:]
        if s.numel() > 1 and float(gap.min()) < (1e-4 if case["mode"] != "raw" else 1e-300):
            return False
        pair = _iou64(c["boxes"], c["boxes"])
        if float((pair - 0.2).abs().min()) < 1e-3:
            return False
        m = mist(*image_inputs(case, i), ids, top_pro)
        if float((_iou64(m["boxes"], case["boxes"][i]) - 0.5).abs().min()) < 1e-4:
            return False
    return True


def generate(rows, classes_per_image, mode, first_seed=0, K=20):
    """The first seed from `first_seed` on whose case is well defined -> (case, seeds tried)."""
    tried = 0
    while True:
        case = make_case(first_seed + tried, rows, classes_per_image, K=K, mode=mode)
        tried += 1
        if well_defined(case):
            return case, tried
        assert tried < 16, "no well-defined case among %d seeds" % tried
