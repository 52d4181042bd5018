"""NumPy restatement of the panoptic-quality arithmetic as DESIGN.md §4f states it (the matching rules of panopticapi's
pq_compute_single_core and its pq_average; the package itself is not available to this suite), and of the semantic
confusion matrix with the four summary metrics.  Written from the statement of the algorithm, not from the device
code: pairs come from `gt * OFFSET + pred` and np.unique with counts, segments live in dictionaries, the confusion
matrix is one np.bincount."""
from collections import OrderedDict

import numpy as np

OFFSET = 1 << 32          # predicted ids are any non-negative int32
VOID = 0


def _counts(values):
    labels, cnt = np.unique(values, return_counts=True)
    return dict(zip(labels.tolist(), cnt.tolist()))


def pq_image(pred, pred_table, num_pred, thing_cat, stuff_cat, gt, gt_table, C):
    """One image -> dict(tp, fp, fn (C,) int64; matches: [(category, iou)] in gt-row order; stats (3,) int64 = {pixels
    naming no row, predicted rows without a pixel, rows whose category is -1 / out of range})."""
    pred = np.asarray(pred).reshape(-1).astype(np.int64)
    gt = np.asarray(gt).reshape(-1).astype(np.int64)
    pred_table = np.asarray(pred_table, np.int64).reshape(-1, 5)
    pred_table = pred_table[:max(0, min(int(num_pred), len(pred_table)))]
    gt_table = np.asarray(gt_table, np.int64).reshape(-1, 2)
    assert pred.shape == gt.shape and (pred >= 0).all()
    tp, fp, fn = (np.zeros(C, np.int64) for _ in range(3))
    stats = np.zeros(3, np.int64)

    def category(cat):
        if 0 <= cat < C:
            return cat
        stats[2] += 1
        return -1

    pred_segms, ownerless = OrderedDict(), 0           # id -> info; rows that can own no pixel (id 0, a repeated id)
    for sid, isthing, k, _, _ in pred_table.tolist():
        cmap = thing_cat if isthing else stuff_cat
        cat = category(int(cmap[k]) if 0 <= k < len(cmap) else -1)
        if sid == VOID or sid in pred_segms:
            ownerless += 1
        else:
            pred_segms[sid] = {"category": cat, "area": 0}
    gt_segms = OrderedDict()
    for r, (cat, crowd) in enumerate(gt_table.tolist()):
        gt_segms[r + 1] = {"category": category(cat), "iscrowd": crowd != 0, "area": 0}

    # counted areas; a value that names no row is counted and becomes VOID
    for values, segms in ((pred, pred_segms), (gt, gt_segms)):
        for label, c in _counts(values).items():
            if label == VOID:
                continue
            if label in segms:
                segms[label]["area"] = c
            else:
                stats[0] += c
                values[values == label] = VOID
    stats[1] = ownerless + sum(1 for s in pred_segms.values() if s["area"] == 0)

    pair = gt.astype(np.uint64) * np.uint64(OFFSET) + pred.astype(np.uint64)
    inter_of = {(label // OFFSET, label % OFFSET): c for label, c in _counts(pair).items()}

    gt_matched, pred_matched, iou_of = set(), set(), {}
    for (g, p), inter in inter_of.items():
        if g == VOID or p == VOID:
            continue
        gs, ps = gt_segms[g], pred_segms[p]
        if gs["iscrowd"] or gs["category"] < 0 or gs["category"] != ps["category"]:
            continue
        union = ps["area"] + gs["area"] - inter - inter_of.get((VOID, p), 0)
        iou = np.float64(inter) / np.float64(union)
        if iou > 0.5:
            assert g not in gt_matched and p not in pred_matched
            tp[gs["category"]] += 1
            gt_matched.add(g)
            pred_matched.add(p)
            iou_of[g] = iou

    crowd_row = {}
    for g, gs in gt_segms.items():
        if g in gt_matched or gs["category"] < 0:
            continue
        if gs["iscrowd"]:
            crowd_row[gs["category"]] = g                # a later crowd row of the category replaces an earlier one
        else:
            fn[gs["category"]] += 1

    for p, ps in pred_segms.items():
        if p in pred_matched or ps["category"] < 0:
            continue
        x = inter_of.get((VOID, p), 0)
        if ps["category"] in crowd_row:
            x += inter_of.get((crowd_row[ps["category"]], p), 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            shielded = np.float64(x) / np.float64(ps["area"]) > 0.5
        if not shielded:
            fp[ps["category"]] += 1

    matches = [(gt_segms[g]["category"], iou_of[g]) for g in sorted(iou_of)]
    return dict(tp=tp, fp=fp, fn=fn, matches=matches, stats=stats)


def pq_accumulate(images, thing_cat, stuff_cat, C):
    """images: iterable of (pred, pred_table, num_pred, gt, gt_table).  -> totals: tp, fp, fn (C,) int64, iou_sum (C,)
    float64 added one match at a time in (image, gt row) order, stats (4,) int64 (the fourth: images)."""
    tot = dict(tp=np.zeros(C, np.int64), fp=np.zeros(C, np.int64), fn=np.zeros(C, np.int64),
               iou_sum=np.zeros(C, np.float64), stats=np.zeros(4, np.int64))
    for pred, pred_table, num_pred, gt, gt_table in images:
        r = pq_image(pred, pred_table, num_pred, thing_cat, stuff_cat, gt, gt_table, C)
        for k in ("tp", "fp", "fn"):
            tot[k] += r[k]
        for cat, iou in r["matches"]:
            tot["iou_sum"][cat] = tot["iou_sum"][cat] + iou
        tot["stats"][:3] += r["stats"]
        tot["stats"][3] += 1
    return tot


def pq_average(tp, fp, fn, iou_sum, isthing):
    """Per category with tp + fp + fn > 0: pq = iou / (tp + fp/2 + fn/2), sq = iou / tp (0 without tp), rq = tp / (tp +
    fp/2 + fn/2); plain means over the counted categories of All / Things / Stuff, NaN for a group with none."""
    out = {}
    for name, want in (("All", None), ("Things", True), ("Stuff", False)):
        pq = sq = rq = 0.0
        n = 0
        for c in range(len(tp)):
            if want is not None and bool(isthing[c]) != want:
                continue
            t, p, f, iou = int(tp[c]), int(fp[c]), int(fn[c]), float(iou_sum[c])
            if t + p + f == 0:
                continue
            n += 1
            pq += iou / (t + 0.5 * p + 0.5 * f)
            sq += iou / t if t != 0 else 0
            rq += t / (t + 0.5 * p + 0.5 * f)
        nan = float("nan")
        out[name] = {"pq": pq / n if n else nan, "sq": sq / n if n else nan, "rq": rq / n if n else nan, "n": n}
    return out


def pq_result_dict(tp, fp, fn, iou_sum, isthing):
    """{"panoptic_seg": {PQ, SQ, RQ, PQ_th, ..., RQ_st}}, values x100."""
    r = pq_average(tp, fp, fn, iou_sum, isthing)
    res = {}
    for suffix, grp in (("", "All"), ("_th", "Things"), ("_st", "Stuff")):
        for m in ("pq", "sq", "rq"):
            res[m.upper() + suffix] = 100 * r[grp][m]
    return OrderedDict({"panoptic_seg": res})


# ------------------------------------------------------------------------------------------------ semantic segmentation
def confusion(pred, gt, num_classes, ignore_label):
    """One image -> (C+1, C+1) int64 counts indexed [pred, gt]; the ignore label takes the extra gt column."""
    side = num_classes + 1
    p = np.asarray(pred).reshape(-1).astype(np.int64)
    g = np.asarray(gt).reshape(-1).astype(np.int64)
    g = np.where(g == ignore_label, num_classes, g)
    return np.bincount(side * p + g, minlength=side * side).reshape(side, side)


def sem_seg_metrics(conf, class_names):
    """mIoU, fwIoU, mACC, pACC and the per-class IoU / ACC (x100) from the confusion matrix without its ignore row and
    column.  A class is scored only where it occurs in the ground truth (NaN otherwise), also for IoU; mIoU divides the
    sum of those IoUs by the number of classes that occur in the ground truth OR the prediction."""
    C = len(class_names)
    m = np.asarray(conf, np.int64)[:C, :C]
    hit = np.diagonal(m).astype(np.float64)
    in_gt = m.sum(axis=0).astype(np.float64)
    in_pred = m.sum(axis=1).astype(np.float64)
    seen_gt = in_gt > 0
    seen_any = (in_gt + in_pred) > 0
    acc = np.full(C, np.nan)
    iou = np.full(C, np.nan)
    acc[seen_gt] = hit[seen_gt] / in_gt[seen_gt]
    iou[seen_gt] = hit[seen_gt] / (in_gt + in_pred - hit)[seen_gt]
    with np.errstate(invalid="ignore", divide="ignore"):
        share = in_gt / np.sum(in_gt)
        res = OrderedDict()
        res["mIoU"] = 100 * (np.sum(iou[seen_gt]) / np.sum(seen_any))
        res["fwIoU"] = 100 * np.sum(iou[seen_gt] * share[seen_gt])
        for i, name in enumerate(class_names):
            res["IoU-" + name] = 100 * iou[i]
        res["mACC"] = 100 * (np.sum(acc[seen_gt]) / np.sum(seen_gt))
        res["pACC"] = 100 * (np.sum(hit) / np.sum(in_gt))
        for i, name in enumerate(class_names):
            res["ACC-" + name] = 100 * acc[i]
    return OrderedDict({"sem_seg": res})
