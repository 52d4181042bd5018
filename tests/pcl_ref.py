"""CPU restatement of PCL's proposal clustering and loss, written from the contract in jtsm_amd/csrc/pcl.hip
(the reference: projects/WSL/wsl/modeling/roi_heads/third_party/pcl.py:24-200 and
projects/WSL/wsl/layers/csrc/pcl_loss/pcl_loss_cpu.cpp:8-115).  One image per call.

Arithmetic: probabilities and IoUs in float32 with every step rounded on its own, k-means means in float64 (summed
exactly), pc_prob and the summed weights in float64 rounded once.  Tie rules (the reference leaves them to an unstable
argsort): LOWEST INDEX among equal degrees, the EARLIER-PICKED centre among equal scores; `info` reports whether a case
met one.  `top_sets` replaces the deterministic Lloyd step by recorded sets (what scikit-learn returned), one array of
pool-relative indices per present class.  Lives under tests/ (oracle/ is frozen)."""
import math

import numpy as np

F = np.float32
CLIP_LO, CLIP_HI = F(1e-9), F(1.0 - 1e-9)
GRAPH_IOU, FG_IOU, BG_IOU = F(0.4), F(0.5), F(0.1)
MAX_PC = 5
LLOYD_PASSES = 300


def clip_probs(p):
    return np.minimum(np.maximum(np.asarray(p, np.float32), CLIP_LO), CLIP_HI)


def pairwise_iou(a, b):
    """(N, M) float32: intersection / (area_a + area_b - intersection), 0 where the boxes do not meet."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    w = np.maximum(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), F(0))
    h = np.maximum(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), F(0))
    inter = (w * h).astype(np.float32)
    aa = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])).astype(np.float32)
    ab = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(np.float32)
    union = ((aa[:, None] + ab[None, :]).astype(np.float32) - inter).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(inter > 0, (inter / union).astype(np.float32), F(0)).astype(np.float32)


def lloyd_top_set(values):
    """Indices (ascending) of the top-ranking set of a 1-D float32 array: the deterministic substitution for
    KMeans(n_clusters=min(3, n), random_state=3)."""
    v32 = np.asarray(values, np.float32).reshape(-1)
    n = v32.shape[0]
    if n <= 1:
        return np.arange(n)
    v = v32.astype(np.float64)
    lo, hi = float(v.min()), float(v.max())
    ctr = np.array([lo, (lo + hi) / 2.0, hi] if n >= 3 else [lo, hi], np.float64)
    asg = np.full(n, -1)
    for _ in range(LLOYD_PASSES):
        new = np.abs(v[:, None] - ctr[None, :]).argmin(axis=1)          # the first minimum: ties to the lower centre
        if np.array_equal(new, asg):
            break
        asg = new
        for k in range(len(ctr)):
            m = asg == k
            if m.any():
                ctr[k] = math.fsum(v[m]) / int(m.sum())
    top = int(np.argmax(ctr))                                           # the first of equal centres
    idx = np.nonzero(asg == top)[0]
    if idx.size == 0:
        idx = np.array([int(np.argmax(v32))])
    return idx


def graph_centres(boxes, prev, im_labels, top_sets=None):
    """-> (centre rows, classes (1-based), scores, info).  prev (R, K) clipped float32; im_labels (K,)."""
    boxes = np.asarray(boxes, np.float32)
    R, K = prev.shape
    pool = np.arange(R)                      # original rows still in the candidate pool, ascending
    rows, classes, scores = [], [], []
    info = {"degree_tie": False, "score_tie": False, "sets": []}
    present = [c for c in range(K) if im_labels[c] == 1]
    for ci, c in enumerate(present):
        if pool.size == 0:
            continue
        col = prev[pool, c]
        rel = np.asarray(top_sets[ci]) if top_sets is not None else lloyd_top_set(col)
        rel = np.sort(rel)
        info["sets"].append(rel)
        members = pool[rel]
        p = col[rel]
        T = members.size
        graph = pairwise_iou(boxes[members], boxes[members]) > GRAPH_IOU
        graph[np.arange(T), np.arange(T)] = True                         # a box has an edge to itself
        alive = np.ones(T, bool)
        keep, keep_scores = [], []
        count = T
        while True:
            deg = (graph & alive[None, :]).sum(axis=1) * alive
            best = int(deg.max())
            if best == 0:
                break
            if (deg == best).sum() > 1:
                info["degree_tie"] = True
            node = int(np.argmax(deg))                                   # lowest index among equal degrees
            nb = graph[node] & alive
            keep.append(node)
            keep_scores.append(p[nb].max())
            alive &= ~nb
            count -= int(nb.sum())
            if count <= 5:
                break
        keep_scores = np.array(keep_scores, np.float32)
        if len(np.unique(keep_scores)) != len(keep_scores):
            info["score_tie"] = True
        order = np.argsort(-keep_scores.astype(np.float64), kind="stable")[:MAX_PC]   # earlier-picked among equals
        chosen = members[np.array(keep)[order]]
        rows += list(chosen)
        classes += [c + 1] * len(chosen)
        scores += list(keep_scores[order])
        pool = pool[~np.isin(pool, chosen)]
    return np.array(rows, np.int64), np.array(classes, np.int32), np.array(scores, np.float32), info


def proposal_clusters(boxes, centre_rows, centre_classes, centre_scores, probs_new):
    """The per-proposal and per-cluster tables.  probs_new (R, K+1) clipped float32, background in column 0."""
    boxes = np.asarray(boxes, np.float32)
    R, G = boxes.shape[0], len(centre_rows)
    labels = np.zeros(R, np.int32)
    assign = np.full(R, -1, np.int32)
    weights = np.zeros(R, np.float32)
    pc_labels = np.asarray(centre_classes, np.int32).copy()
    pc_count = np.zeros(G, np.int32)
    pc_weight = np.zeros(G, np.float32)
    pc_probs = np.zeros(G, np.float32)
    if G:
        ov = pairwise_iou(boxes, boxes[centre_rows])
        a = ov.argmax(axis=1)                                            # the first maximum
        mx = ov[np.arange(R), a]
        weights = np.where(mx < BG_IOU, F(0), centre_scores[a]).astype(np.float32)
        fg = ~(mx < FG_IOU)
        labels = np.where(fg, pc_labels[a], 0).astype(np.int32)
        assign = np.where(fg, a, -1).astype(np.int32)
        for j in range(G):
            m = assign == j
            pc_count[j] = int(m.sum())
            if pc_count[j]:
                pc_weight[j] = F(float(centre_scores[j]) * int(pc_count[j]))
                pc_probs[j] = F(math.fsum(probs_new[m, pc_labels[j]].astype(np.float64)) / int(pc_count[j]))
    return {"labels": labels, "cls_loss_weights": weights, "gt_assignment": assign, "pc_labels": pc_labels,
            "pc_probs": pc_probs, "pc_count": pc_count, "img_cls_loss_weights": pc_weight}


def pcl(boxes, cls_prob, im_labels, cls_prob_new, top_sets=None):
    """PCL() of one image: cls_prob (R, K) or (R, K+1) with the background first; im_labels (K,) or (1, K);
    cls_prob_new (R, K+1).  -> the tables (+ "centre_rows", "centre_scores", "info")."""
    im_labels = np.asarray(im_labels).reshape(-1)
    cls_prob = np.asarray(cls_prob, np.float32)
    if cls_prob.shape[1] != im_labels.shape[0]:
        cls_prob = cls_prob[:, 1:]
    prev, new = clip_probs(cls_prob), clip_probs(cls_prob_new)
    rows, classes, scores, info = graph_centres(boxes, prev, im_labels, top_sets)
    out = proposal_clusters(boxes, rows, classes, scores, new)
    b = np.asarray(boxes, np.float32)
    info["duplicate_box"] = len(np.unique(b, axis=0)) != len(b)
    out.update(centre_rows=rows, centre_scores=scores, info=info,
               im_labels_real=np.concatenate([[1], im_labels]).astype(np.float32))
    return out


def softmax(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def loss(probs, t):
    """The PCL loss of one image from its probabilities (R, K+1) and tables, in float64."""
    p = np.asarray(probs, np.float64)
    R = p.shape[0]
    bg = t["labels"] == 0
    out = -np.sum(t["cls_loss_weights"][bg].astype(np.float64) * np.log(np.maximum(p[bg, 0], 1e-6)))
    for j in range(len(t["pc_labels"])):
        if t["pc_count"][j] > 0:
            out -= float(t["img_cls_loss_weights"][j]) * math.log(max(float(t["pc_probs"][j]), 1e-6))
    return out / R


def loss_grad_logits(logits, t, upstream=1.0, images=1):
    """d loss / d logits (R, K+1) in float64: the reference's gradient to the probabilities carried through the
    soft-max, times upstream / images."""
    p = softmax(logits)
    R = p.shape[0]
    g = np.zeros_like(p)
    lab = t["labels"]
    bg = lab == 0
    g[bg, 0] = -t["cls_loss_weights"][bg].astype(np.float64) / np.maximum(p[bg, 0], 1e-5)
    for r in np.nonzero(~bg)[0]:
        j = t["gt_assignment"][r]
        g[r, lab[r]] = -float(t["img_cls_loss_weights"][j]) / max(float(t["pc_count"][j]) * float(t["pc_probs"][j]), 1e-5)
    g *= upstream / (R * images)
    return p * (g - (g * p).sum(axis=1, keepdims=True))
