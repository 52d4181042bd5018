"""A literal NumPy / Python restatement of COCO box / mask AP as DESIGN.md §4g fixes it: what the reference's
COCOEvaluator computes through pycocotools' COCOeval parameters and data preparation, pycocotools' bbIou / rleIou
(restated: the package is not installed here) and the reference's own detectron2/layers/csrc/cocoeval/cocoeval.cpp
(EvaluateImages, Accumulate), which tests/golden/coco_eval_reference.npz pins bit for bit.  Plain loops, one IEEE
operation per line of arithmetic, Python floats (fp64) throughout.

A dataset here is a list of images in process() order, each a dict:
  image_id; det_boxes (n,4) float32 XYXY, det_scores (n,) float32, det_classes (n,) int, det_masks (n,H,W) bool or None;
  gt_cats (G,) int, gt_boxes (G,4) float64 XYWH, gt_area (G,) float64, gt_crowd (G,) 0/1, gt_masks (G,H,W) bool or None.
"""
from bisect import bisect_left
from collections import OrderedDict

import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
METRICS = ["AP", "AP50", "AP75", "APs", "APm", "APl"]


def detections_of(image, task):
    """instances_to_coco_json + loadRes: per detection (category, score, area, XYWH box as Python floats), Instances
    row order.  BoxMode.convert subtracts on the fp32 array; tolist() widens."""
    b = np.array(image["det_boxes"], dtype=np.float32).reshape(-1, 4).copy()
    b[:, 2] -= b[:, 0]
    b[:, 3] -= b[:, 1]
    boxes = b.tolist()
    scores = np.asarray(image["det_scores"], dtype=np.float32).tolist()
    out = []
    for k in range(len(scores)):
        if task == "segm":
            area = float(int(np.asarray(image["det_masks"][k], dtype=bool).sum()))
        else:
            area = boxes[k][2] * boxes[k][3]
        out.append(dict(row=k, cat=int(image["det_classes"][k]), score=scores[k], area=area, box=boxes[k]))
    return out


def stable_order(scores):
    """Indices by descending score, ties in input order (np.argsort(-s, kind='mergesort') / std::stable_sort with >)."""
    return sorted(range(len(scores)), key=lambda j: -scores[j])


def box_iou(d, g, crowd):
    dx, dy, dw, dh = d
    gx, gy, gw, gh = g
    ga = gw * gh
    da = dw * dh
    w = min(dw + dx, gw + gx) - max(dx, gx)
    if w <= 0:
        return 0.0
    h = min(dh + dy, gh + gy) - max(dy, gy)
    if h <= 0:
        return 0.0
    i = w * h
    u = da if crowd else da + ga - i
    return i / u


def mask_iou(d, g, crowd):
    d, g = np.asarray(d, dtype=bool), np.asarray(g, dtype=bool)
    i = int((d & g).sum())
    if i == 0:
        return 0.0
    a_dt, a_gt = int(d.sum()), int(g.sum())
    u = a_dt if crowd else a_dt + a_gt - i
    return float(i) / float(u)


def evaluate_image_category(dets, gts, ious, area_rng, iou_thrs):
    """MatchDetectionsToGroundTruth for one (image, category, area range).  dets: the score-ordered, truncated list
    (dicts with area); gts: dicts with area, crowd (ignore := crowd) in annotation order; ious[d][g] by sorted detection
    position and annotation-order ground truth.  -> (detection_matches (T,D) ids = the ground truth's row in the image
    + 1 (its `id`; without one its position here + 1) or 0, detection_ignores
    (T,D), ground_truth_ignores (G) in the sorted order)."""
    lo, hi = area_rng
    ignores = [bool(g["crowd"]) or g["area"] < lo or g["area"] > hi for g in gts]
    gsort = sorted(range(len(gts)), key=lambda j: int(ignores[j]))
    G, D, T = len(gts), len(dets), len(iou_thrs)
    gt_matches = [[0] * G for _ in range(T)]
    dt_matches = [[0] * D for _ in range(T)]
    dt_ignores = [[False] * D for _ in range(T)]
    gt_ignores = [ignores[j] for j in gsort]
    for t in range(T):
        for d in range(D):
            best = min(float(iou_thrs[t]), 1 - 1e-10)
            match = -1
            for g in range(G):
                if gt_matches[t][g] > 0 and not gts[gsort[g]]["crowd"]:
                    continue
                if match >= 0 and not gt_ignores[match] and gt_ignores[g]:
                    break
                if ious[d][gsort[g]] >= best:
                    best = ious[d][gsort[g]]
                    match = g
            if match >= 0:
                dt_ignores[t][d] = gt_ignores[match]
                dt_matches[t][d] = gts[gsort[match]].get("id", gsort[match] + 1)
                gt_matches[t][match] = d + 1
            dt_ignores[t][d] = dt_ignores[t][d] or (dt_matches[t][d] == 0
                                                    and (dets[d]["area"] < lo or dets[d]["area"] > hi))
    return dt_matches, dt_ignores, gt_ignores


def evaluate_images(dataset, task, num_categories, iou_thrs=IOU_THRS, area_rng=AREA_RNG, max_det=MAX_DETS[-1]):
    """COCOeval_opt.evaluate: -> (image order = ascending image id as indices into `dataset`, evals[(i, c, a)] =
    dict(scores, matches, ignores, gt_ignores) with i the position in that order, per_image[i] = dict(rank (n,) with -1
    beyond max_det, ious {c: (D, G_c) list of rows}, gt_rows {c: annotation rows}, det_rows {c: Instances rows})."""
    order = sorted(range(len(dataset)), key=lambda j: dataset[j]["image_id"])
    evals, per_image = {}, []
    for i, j in enumerate(order):
        image = dataset[j]
        dets = detections_of(image, task)
        n = len(dets)
        rank = np.full(n, -1, np.int64)
        info = dict(rank=rank, ious={}, gt_rows={}, det_rows={})
        for c in range(num_categories):
            mine = [d for d in dets if d["cat"] == c]
            mine = [mine[k] for k in stable_order([d["score"] for d in mine])][:max_det]
            for r, d in enumerate(mine):
                rank[d["row"]] = r
            rows = [g for g in range(len(image["gt_cats"])) if int(image["gt_cats"][g]) == c]
            gts = [dict(id=g + 1, area=float(image["gt_area"][g]), crowd=bool(image["gt_crowd"][g])) for g in rows]
            ious = []
            for d in mine:
                if task == "segm":
                    ious.append([mask_iou(image["det_masks"][d["row"]], image["gt_masks"][g], bool(image["gt_crowd"][g]))
                                 for g in rows])
                else:
                    ious.append([box_iou(d["box"], [float(v) for v in image["gt_boxes"][g]], bool(image["gt_crowd"][g]))
                                 for g in rows])
            info["ious"][c], info["gt_rows"][c], info["det_rows"][c] = ious, rows, [d["row"] for d in mine]
            for a, rng in enumerate(area_rng):
                m, ig, gig = evaluate_image_category(mine, gts, ious, rng, iou_thrs)
                evals[(i, c, a)] = dict(scores=[d["score"] for d in mine], matches=m, ignores=ig, gt_ignores=gig)
        per_image.append(info)
    return order, evals, per_image


def accumulate(evals, num_images, num_categories, iou_thrs=IOU_THRS, rec_thrs=REC_THRS, max_dets=MAX_DETS,
               num_areas=len(AREA_RNG)):
    """Accumulate of cocoeval.cpp: -> precision, scores (T,R,K,A,M) and recall (T,K,A,M) float64, and npos (K,A)."""
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), num_categories, num_areas, len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    npos_table = np.zeros((K, A), np.int64)
    rec_list = [float(v) for v in rec_thrs]
    for c in range(K):
        for a in range(A):
            for m, max_det in enumerate(max_dets):
                ev_idx, det_idx, det_scores = [], [], []
                npos = 0
                for i in range(num_images):
                    e = evals[(i, c, a)]
                    for d in range(min(len(e["scores"]), max_det)):
                        ev_idx.append(i)
                        det_idx.append(d)
                        det_scores.append(e["scores"][d])
                    npos += sum(1 for g in e["gt_ignores"] if not g)
                npos_table[c, a] = npos
                order = stable_order(det_scores)
                if npos == 0:
                    continue
                for t in range(T):
                    tp = fp = 0
                    precs, recs = [], []
                    for s in order:
                        e = evals[(ev_idx[s], c, a)]
                        match, ignore = e["matches"][t][det_idx[s]], e["ignores"][t][det_idx[s]]
                        if match > 0 and not ignore:
                            tp += 1
                        if match == 0 and not ignore:
                            fp += 1
                        recs.append(float(tp) / npos)
                        precs.append(float(tp) / (tp + fp) if tp + fp > 0 else 0.0)
                    recall[t, c, a, m] = recs[-1] if recs else 0
                    for i in range(len(precs) - 1, 0, -1):
                        if precs[i] > precs[i - 1]:
                            precs[i - 1] = precs[i]
                    for r, thr in enumerate(rec_list):
                        k = bisect_left(recs, thr)
                        if k < len(precs):
                            precision[t, r, c, a, m] = precs[k]
                            scores[t, r, c, a, m] = det_scores[order[k]]
                        else:
                            precision[t, r, c, a, m] = 0
                            scores[t, r, c, a, m] = 0
    return precision, scores, recall, npos_table


def summarize(precision, recall, iou_thrs=IOU_THRS, max_dets=MAX_DETS):
    """pycocotools' _summarizeDets: the twelve stats (six AP, six AR)."""
    def one(ap, iou=None, area=0, max_det=max_dets[-1]):
        m = max_dets.index(max_det)
        s = precision[:, :, :, area, m] if ap else recall[:, :, area, m]
        if iou is not None:
            s = s[np.where(iou == iou_thrs)[0]]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    return np.array([one(1), one(1, iou=.5), one(1, iou=.75), one(1, area=1), one(1, area=2), one(1, area=3),
                     one(0, max_det=max_dets[0]), one(0, max_det=max_dets[1]), one(0), one(0, area=1), one(0, area=2),
                     one(0, area=3)], dtype=np.float64)


def derive_results(stats, precision, class_names=None):
    """_derive_coco_results (coco_evaluation.py:288-354) without the logging."""
    if stats is None:
        return {metric: float("nan") for metric in METRICS}
    results = {metric: float(stats[idx] * 100 if stats[idx] >= 0 else "nan") for idx, metric in enumerate(METRICS)}
    if class_names is None or len(class_names) <= 1:
        return results
    assert len(class_names) == precision.shape[2]
    for idx, name in enumerate(class_names):
        p = precision[:, :, idx, 0, -1]
        p = p[p > -1]
        results["AP-" + "{}".format(name)] = float((np.mean(p) if p.size else float("nan")) * 100)
    return results


def evaluate(dataset, num_categories, tasks=("bbox",), class_names=None):
    """-> (result dict as COCOEvaluator.evaluate's, tables {task: dict(precision, scores, recall, npos, stats, order,
    evals, per_image)})."""
    results, tables = OrderedDict(), {}
    for task in tasks:
        order, evals, per_image = evaluate_images(dataset, task, num_categories)
        precision, scores, recall, npos = accumulate(evals, len(dataset), num_categories)
        stats = summarize(precision, recall)
        any_det = any(len(im["det_scores"]) for im in dataset)
        results[task] = derive_results(stats if any_det else None, precision, class_names)
        tables[task] = dict(precision=precision, scores=scores, recall=recall, npos=npos, stats=stats, order=order,
                            evals=evals, per_image=per_image)
    return results, tables


def match_bits(evals, i, c, num_dets, num_thrs=len(IOU_THRS), num_areas=len(AREA_RNG)):
    """The device's record words of the detections of (image i, category c) by rank: bit a * T + t of `matched` /
    `ignore` from evals[(i, c, a)]."""
    matched, ignore = [0] * num_dets, [0] * num_dets
    for a in range(num_areas):
        e = evals[(i, c, a)]
        for t in range(num_thrs):
            for d in range(num_dets):
                if e["matches"][t][d] > 0:
                    matched[d] |= 1 << (a * num_thrs + t)
                if e["ignores"][t][d]:
                    ignore[d] |= 1 << (a * num_thrs + t)
    return matched, ignore


# ---------------------------------------------------------------------------------------------- recorded cases
def dataset_to_fields(dataset):
    """A dataset as flat arrays for an npz (masks as packed bits, row-major, np.packbits' default bit order)."""
    cat = lambda rows, dt, shape: (np.concatenate([np.asarray(r, dt).reshape(shape) for r in rows])  # noqa: E731
                                   if rows else np.zeros(shape, dt).reshape((0,) + tuple(shape[1:])))
    f = dict(image_ids=np.array([im["image_id"] for im in dataset], np.int64),
             det_count=np.array([len(im["det_scores"]) for im in dataset], np.int64),
             gt_count=np.array([len(im["gt_cats"]) for im in dataset], np.int64),
             det_boxes=cat([im["det_boxes"] for im in dataset], np.float32, (-1, 4)),
             det_scores=cat([im["det_scores"] for im in dataset], np.float32, (-1,)),
             det_classes=cat([im["det_classes"] for im in dataset], np.int64, (-1,)),
             gt_cats=cat([im["gt_cats"] for im in dataset], np.int64, (-1,)),
             gt_boxes=cat([im["gt_boxes"] for im in dataset], np.float64, (-1, 4)),
             gt_area=cat([im["gt_area"] for im in dataset], np.float64, (-1,)),
             gt_crowd=cat([im["gt_crowd"] for im in dataset], np.uint8, (-1,)))
    if dataset and dataset[0]["det_masks"] is not None:
        H, W = dataset[0]["det_masks"].shape[1:]
        f["mask_hw"] = np.array([H, W], np.int64)
        bits = lambda key: np.packbits(np.concatenate(  # noqa: E731
            [np.asarray(im[key], bool).reshape(-1, H * W) for im in dataset]), axis=1)
        f["det_mask_bits"], f["gt_mask_bits"] = bits("det_masks"), bits("gt_masks")
    return f


def dataset_from_fields(f):
    masks = "mask_hw" in f
    if masks:
        H, W = (int(v) for v in f["mask_hw"])
        unpack = lambda b: np.unpackbits(b, axis=1)[:, :H * W].astype(bool).reshape(-1, H, W)  # noqa: E731
        dm, gm = unpack(f["det_mask_bits"]), unpack(f["gt_mask_bits"])
    dataset, d0, g0 = [], 0, 0
    for i, image_id in enumerate(f["image_ids"]):
        d1, g1 = d0 + int(f["det_count"][i]), g0 + int(f["gt_count"][i])
        dataset.append(dict(
            image_id=int(image_id), det_boxes=f["det_boxes"][d0:d1], det_scores=f["det_scores"][d0:d1],
            det_classes=f["det_classes"][d0:d1], det_masks=dm[d0:d1] if masks else None, gt_cats=f["gt_cats"][g0:g1],
            gt_boxes=f["gt_boxes"][g0:g1], gt_area=f["gt_area"][g0:g1], gt_crowd=f["gt_crowd"][g0:g1],
            gt_masks=gm[g0:g1] if masks else None))
        d0, g0 = d1, g1
    return dataset


def flatten_evals(evals, num_images, num_categories, num_areas=len(AREA_RNG)):
    """The per-(category, area range, image) results in cocoeval.cpp's results_all order as flat arrays: sizes (E,2) =
    (D, G), matches and ignores (sum of T D), gt_ignores (sum of G)."""
    sizes, matches, ignores, gt_ignores = [], [], [], []
    for c in range(num_categories):
        for a in range(num_areas):
            for i in range(num_images):
                e = evals[(i, c, a)]
                sizes.append([len(e["scores"]), len(e["gt_ignores"])])
                matches += [v for row in e["matches"] for v in row]
                ignores += [v for row in e["ignores"] for v in row]
                gt_ignores += list(e["gt_ignores"])
    return (np.array(sizes, np.int64).reshape(-1, 2), np.array(matches, np.int64), np.array(ignores, bool),
            np.array(gt_ignores, bool))
