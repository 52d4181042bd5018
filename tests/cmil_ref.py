"""NumPy restatement of C-MIL's two host operators, loop for loop:

    ROIMerge_forward_cpu / ROIMerge_backward_cpu   projects/WSL/wsl/layers/csrc/ROIMerge/ROIMerge_cpu.cpp:33-232, :234-287
    getlambda                                      :11-17
    ROILabel_forward_cpu                           projects/WSL/wsl/layers/csrc/ROILabel/ROILabel_cpu.cpp:59-161

The reference sources include TH/TH.h, which the installed torch no longer ships, so the oracle does not build them;
tests/golden/make_cmil_golden.py compiled them once with an empty stand-in for that header and recorded
tests/golden/cmil_reference_cases.npz, which pins this restatement (tests/test_cmil_ref.py) and the device
(tests/test_hip_cmil.py) to the reference's own results.  Two things the reference leaves open are made explicit:
  * std::sort on the scores (:26-28) leaves the order of equal scores open: here equal scores go by lower row;
  * std::random_shuffle under srand(time(0)) (ROILabel :110-118): the visiting order `perm` is an input.
J / U, the R x R IoU matrices the reference is handed, are pairwise_iou in float32 with every step rounded on its own.
A class whose rows have run out gets no seed (the reference would push row -1 and index with it); an image without a
seed labels every row num_classes with weight 0; fg < bg_hi is refused.

Also the generator of the piled cases the GPU tests run, with the conditions under which the integer results are well
defined asserted in float64."""
import math

import numpy as np

TOP, WINDOW = 200, 40            # ROIMerge_cpu.cpp:105, :116
FLT_MAX = np.float32(np.finfo(np.float32).max)


def getlambda(cur_iter, size_epoch, max_epoch):
    """(:11-17) at iter = cur_iter / size_epoch, in double, rounded once to float32."""
    low = 0.01
    it = float(cur_iter) / float(size_epoch)
    return np.float32((math.log(it + low) - math.log(low)) / (math.log(float(max_epoch) + low) - math.log(low)))


def pairwise_iou(a, b, dtype=np.float32):
    """detectron2.structures.pairwise_iou of (n, 4) and (m, 4) xyxy boxes, every step rounded in `dtype`."""
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.maximum(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), dtype(0))
    h = np.maximum(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), dtype(0))
    inter = w * h
    union = area_a[:, None] + area_b[None, :] - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(inter > 0, inter / union, dtype(0)).astype(dtype)


def merge_ids(S, J, lam):
    """The clique of every row of one image (:91-160) -> (I (n,) int32, number of cliques, cliques among the top)."""
    S = np.asarray(S, np.float32).reshape(-1)
    lam = np.float32(lam)
    n = S.shape[0]
    I = np.full(n, -1, np.int32)
    sort_idx = sorted(range(n), key=lambda i: (-float(S[i]), i))     # descending, equal scores by lower row
    cur_id = 0
    top_k = min(n, TOP)
    for t in range(top_k):
        if I[sort_idx[t]] != -1:
            continue
        I[sort_idx[t]] = cur_id
        end_num = min(t + WINDOW, top_k)
        for tt in range(t, end_num):
            i = sort_idx[tt]
            if I[i] != -1:
                continue
            flag_in_clique = True
            for ttt in range(t, end_num):
                j = sort_idx[ttt]
                if I[j] != cur_id:
                    continue
                if J[i, j] < lam:
                    flag_in_clique = False
                    break
            if flag_in_clique:
                I[i] = cur_id
        cur_id += 1
    num_top_id = cur_id
    for r in range(n):
        if I[r] == -1:
            I[r] = cur_id
            cur_id += 1
    return I, cur_id, num_top_id


class TopIoU(object):
    """J[i, j] for the rows the walk can reach — the first 200 of the order — without building the R x R matrix."""

    def __init__(self, S, boxes):
        S = np.asarray(S, np.float32).reshape(-1)
        top = sorted(range(S.shape[0]), key=lambda i: (-float(S[i]), i))[:TOP]
        self.pos = {r: k for k, r in enumerate(top)}
        bx = np.asarray(boxes, np.float32)[top]
        self.J = pairwise_iou(bx, bx)

    def __getitem__(self, ij):
        return self.J[self.pos[ij[0]], self.pos[ij[1]]]


def merge_means(C, D, I, num_id):
    """(:162-203) -> (MC, MD (num_id, K) float32, IC (num_id,) int32): quotients rounded, added in ascending rows."""
    C, D = np.asarray(C, np.float32), np.asarray(D, np.float32)
    IC = np.bincount(I, minlength=num_id).astype(np.int32)
    MC = np.zeros((num_id, C.shape[1]), np.float32)
    MD = np.zeros((num_id, C.shape[1]), np.float32)
    for r in range(C.shape[0]):
        cnt = np.float32(IC[I[r]])
        MC[I[r]] = MC[I[r]] + C[r] / cnt
        MD[I[r]] = MD[I[r]] + D[r] / cnt
    return MC, MD, IC


def roi_merge(S, boxes, C, D, offsets, lam):
    """ROIMerge over a batch, per image, compacted as the device writes it.  -> dict(MC, MD (R, K) with zero rows behind
    merged_offsets[-1], I (R,) merged rows, IC (R,) per merged row, merged_offsets (B+1,), num_top (B,))."""
    C, D = np.asarray(C, np.float32), np.asarray(D, np.float32)
    R, K = C.shape
    out = dict(MC=np.zeros((R, K), np.float32), MD=np.zeros((R, K), np.float32), I=np.zeros(R, np.int32),
               IC=np.zeros(R, np.int32), merged_offsets=np.zeros(len(offsets), np.int32), num_top=[])
    base = 0
    for b in range(len(offsets) - 1):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        I, num_id, num_top = merge_ids(S[lo:hi], TopIoU(S[lo:hi], boxes[lo:hi]), lam)
        MC, MD, IC = merge_means(C[lo:hi], D[lo:hi], I, num_id)
        out["I"][lo:hi] = I + base
        out["MC"][base:base + num_id], out["MD"][base:base + num_id], out["IC"][base:base + num_id] = MC, MD, IC
        out["num_top"].append(num_top)
        base += num_id
        out["merged_offsets"][b + 1] = base
    return out


def roi_merge_backward(gMC, gMD, I, IC):
    """(:278-284): dC[n] = gMC[I[n]] / IC[I[n]]."""
    cnt = IC[I].astype(np.float32)[:, None]
    return (np.asarray(gMC, np.float32)[I] / cnt).astype(np.float32), (np.asarray(gMD, np.float32)[I] / cnt).astype(np.float32)


def label_seeds(S, class_ids, top_k=1):
    """(:84-108) -> (rows, classes, scores) of the seeds in picking order."""
    S = np.asarray(S, np.float32)
    highest_n, highest_c, highest_p = [], [], []
    for c in class_ids:
        for _ in range(top_k):
            max_pred, max_idx = -FLT_MAX, -1
            for r in range(S.shape[0]):
                if max_pred < S[r, c] and r not in highest_n:
                    max_pred, max_idx = S[r, c], r
            if max_idx < 0:
                continue                    # the rows have run out: no seed
            highest_n.append(max_idx)
            highest_c.append(int(c))
            highest_p.append(max_pred)
    return highest_n, highest_c, highest_p


def roi_label_image(S, boxes, class_ids, CW, perm, fg=0.6, bg_hi=0.4, bg_lo=0.1, num_pos=32, num_neg=96, top_k=1,
                    num_classes=None, seeds=None):
    """ROILabel for one image.  S (n, >= K) class scores, class_ids the present classes ascending, CW (K,) or None,
    perm a permutation of range(n).  seeds: (rows, classes, scores) to use in place of the picking (a frozen choice).
    -> dict(labels (n,) int32, weights (n,) float32, seed_rows, iou (n,) the matched IoU, eligible (fg, bg) counts)."""
    if not fg >= bg_hi:
        raise ValueError("fg_thresh %r is below bg_thresh_hi %r" % (fg, bg_hi))
    S = np.asarray(S, np.float32)
    boxes = np.asarray(boxes, np.float32)
    n = S.shape[0]
    if num_classes is None:
        num_classes = len(CW)
    fg, bg_hi, bg_lo = np.float32(fg), np.float32(bg_hi), np.float32(bg_lo)
    highest_n, highest_c, highest_p = seeds if seeds is not None else label_seeds(S, class_ids, top_k)
    RL, RW = np.zeros(n, np.int32), np.zeros(n, np.float32)
    best = np.zeros(n, np.float32)
    n_pos = n_neg = 0
    U = pairwise_iou(boxes, boxes[highest_n]) if highest_n else np.zeros((n, 0), np.float32)
    for r in perm:
        r = int(r)
        max_iou, max_idx = -FLT_MAX, -1
        for i in range(len(highest_n)):
            if max_iou < U[r, i]:
                max_iou, max_idx = U[r, i], i
        if max_idx < 0:
            RL[r], RW[r] = num_classes, 0.0
            continue
        assign_c = highest_c[max_idx]
        assign_w = np.float32(CW[assign_c]) if CW is not None else highest_p[max_idx]
        if max_iou >= fg and n_pos <= num_pos:
            n_pos += 1
        elif max_iou >= bg_lo and max_iou < bg_hi and n_neg <= num_neg:
            assign_c = num_classes
            n_neg += 1
        else:
            assign_w = np.float32(0)
        RL[r], RW[r], best[r] = assign_c, assign_w, max_iou
    eligible = (int((best >= fg).sum()), int(((best >= bg_lo) & (best < bg_hi)).sum())) if highest_n else (0, 0)
    return dict(labels=RL, weights=RW, seed_rows=list(highest_n), iou=best, eligible=eligible)


# ---- the piled cases of the GPU tests ---------------------------------------------------------------------------------
def piled_boxes(rng, n, size=256.0):
    """n boxes piled on 4 rectangles: jittered copies, so that IoUs spread over (0, 1) inside a pile; every tenth box an
    exact copy of an earlier one (IoU exactly 1: lam = 1 merges something)."""
    anchors = np.array([[20, 30, 120, 140], [90, 60, 230, 200], [40, 120, 160, 250], [130, 20, 250, 110]], np.float64)
    which = rng.integers(0, 4, n)
    jit = rng.uniform(-1, 1, (n, 4)) * rng.choice([2.0, 8.0, 25.0], (n, 1))
    b = anchors[which] + jit
    b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 4)
    b = np.clip(b, 0, size).astype(np.float32)
    for r in range(10, n, 10):
        b[r] = b[rng.integers(0, r)]
    return b


def spread(rng, shape):
    """float32 values of (0, 1), distinct down each column by construction: a shuffled ladder with jittered rungs
    (8300 independent uniform float32 draws would collide about twice per column)."""
    n = shape[0]
    cols = shape[1] if len(shape) > 1 else 1
    v = np.stack([(rng.permutation(n) + rng.uniform(0.1, 0.9, n)) / n for _ in range(cols)], 1).astype(np.float32)
    return v if len(shape) > 1 else v[:, 0]


def tie_free(v):
    v = np.asarray(v).reshape(-1)
    return np.unique(v).size == v.size


def far_from(iou32, boxes_a, boxes_b, thresholds, margin=1e-6):
    """No IoU (evaluated in float64) lies within `margin` of a threshold, except where it equals the threshold exactly
    in float32 too (identical boxes at 1, disjoint boxes at 0: decided without rounding)."""
    iou64 = pairwise_iou(boxes_a, boxes_b, np.float64)
    for t in thresholds:
        near = np.abs(iou64 - float(t)) < margin
        exact = (iou32 == np.float32(t)) & (iou64 == float(t))
        if np.any(near & ~exact):
            return False
    return True


def merge_case(seed, rows, K, lam):
    """Inputs of one ROIMerge case (rows: list of rows per image) whose result is well defined, or None."""
    rng = np.random.default_rng(seed)
    R = int(sum(rows))
    offsets = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    boxes = np.concatenate([piled_boxes(rng, n) for n in rows]) if R else np.zeros((0, 4), np.float32)
    S = np.concatenate([spread(rng, (n,)) for n in rows])
    C = rng.normal(0, 2, (R, K)).astype(np.float32)
    D = rng.normal(0, 2, (R, K)).astype(np.float32)
    for b in range(len(rows)):
        lo, hi = offsets[b], offsets[b + 1]
        if not tie_free(S[lo:hi]):
            return None
        top = np.argsort(-S[lo:hi], kind="stable")[:TOP]
        bx = boxes[lo:hi][top]
        if not far_from(pairwise_iou(bx, bx), bx, bx, [lam]):
            return None
    return dict(S=S, boxes=boxes, C=C, D=D, offsets=offsets, lam=np.float32(lam), rows=list(rows))


def label_case(seed, rows, n_classes_present, K=20, mode="raw"):
    """Inputs of one ROILabel case, or None.  mode: `raw` (scores in [0, 1)) or `logits` ((R, K+1) logits)."""
    rng = np.random.default_rng(seed)
    R, B = int(sum(rows)), len(rows)
    offsets = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    boxes = np.concatenate([piled_boxes(rng, n) for n in rows])
    if mode == "raw":
        S = np.concatenate([spread(rng, (n, K)) for n in rows])
    else:
        S = np.concatenate([spread(rng, (n, K + 1)) for n in rows]) * np.float32(12) - np.float32(6)
    classes = np.zeros((B, K), np.int32)
    counts = np.zeros(B, np.int32)
    for b in range(B):
        ids = np.sort(rng.choice(K, n_classes_present, replace=False))
        classes[b, :len(ids)], counts[b] = ids, len(ids)
        lo, hi = offsets[b], offsets[b + 1]
        if not all(tie_free(S[lo:hi, c]) for c in ids):
            return None
    CW = rng.uniform(0.05, 0.95, (B, K)).astype(np.float32)
    perm = np.concatenate([rng.permutation(n) for n in rows]).astype(np.int32)
    return dict(S=S, boxes=boxes, offsets=offsets, classes=classes, counts=counts, CW=CW, perm=perm, rows=list(rows),
                K=K, mode=mode)
