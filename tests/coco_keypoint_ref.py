"""A literal NumPy / Python restatement of the COCO keypoints task (OKS) as DESIGN.md §4g fixes it: pycocotools'
Params.setKpParams, _prepare (ignore := iscrowd or num_keypoints == 0), computeOks and _summarizeKps — restated from
the published source: the package is not installed here — around the matching and accumulation of
tests/coco_eval_ref.py (the reference's cocoeval.cpp, restated there), which are imported and not copied.
tests/golden/coco_keypoint_reference.npz pins matching and accumulation to the compiled cocoeval.cpp.

The imported matcher takes one `crowd` flag per object and derives `ignore` from it or from an area outside the range.
The keypoints task has two flags (cocoeval.h: InstanceAnnotation.is_crowd / .ignore): an object that is ignored but no
crowd is handed over with area -inf, which lies below every range — ignored in each of them, and matched at most once.

A dataset is coco_eval_ref's list of images, each with three more fields: det_keypoints (n,P,3) float32 (x, y, score as
the model leaves them), gt_keypoints (G,P,3) float64 (x, y, v as the COCO JSON holds them), gt_num_keypoints (G,) int.
"""
import numpy as np

import coco_eval_ref as CR

IOU_THRS, REC_THRS = CR.IOU_THRS, CR.REC_THRS
MAX_DETS = [20]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
METRICS = ["AP", "AP50", "AP75", "APm", "APl"]
COCO_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
MARGIN = 1e-9


def detections_of(image):
    """instances_to_coco_json + loadRes for the keypoints task: coco_eval_ref's bbox detections (the area is the fp32
    XYWH box's w * h: loadRes tests for `bbox` first) plus `keypoints`, the flat list of 3 P doubles — x and y minus
    0.5 in fp32 on a copy, then widened by tolist()."""
    out = CR.detections_of(image, "bbox")
    if not out:
        return out
    k = np.array(image["det_keypoints"], dtype=np.float32).copy()
    k = k.reshape(len(out), -1, 3)
    k[:, :, :2] -= 0.5
    for d, row in zip(out, k):
        d["keypoints"] = row.flatten().tolist()
    return out


def compute_oks(dts, gts, sigmas):
    """pycocotools' COCOeval.computeOks for the score-ordered, truncated detections and the ground truth of one (image,
    category): dts dicts with keypoints; gts dicts with keypoints, bbox (XYWH) and area.  -> (D, G) array."""
    if len(gts) == 0 or len(dts) == 0:
        return []
    ious = np.zeros((len(dts), len(gts)))
    sigmas = np.asarray(sigmas, dtype=np.float64)
    vars = (sigmas * 2) ** 2
    k = len(sigmas)
    for j, gt in enumerate(gts):
        g = np.array(gt['keypoints'])
        xg = g[0::3]; yg = g[1::3]; vg = g[2::3]  # noqa: E702
        k1 = np.count_nonzero(vg > 0)
        bb = gt['bbox']
        x0 = bb[0] - bb[2]; x1 = bb[0] + bb[2] * 2  # noqa: E702
        y0 = bb[1] - bb[3]; y1 = bb[1] + bb[3] * 2  # noqa: E702
        for i, dt in enumerate(dts):
            d = np.array(dt['keypoints'])
            xd = d[0::3]; yd = d[1::3]  # noqa: E702
            if k1 > 0:
                dx = xd - xg
                dy = yd - yg
            else:
                z = np.zeros((k))
                dx = np.max((z, x0 - xd), axis=0) + np.max((z, xd - x1), axis=0)
                dy = np.max((z, y0 - yd), axis=0) + np.max((z, yd - y1), axis=0)
            e = (dx ** 2 + dy ** 2) / vars / (gt['area'] + np.spacing(1)) / 2
            if k1 > 0:
                e = e[vg > 0]
            ious[i, j] = np.sum(np.exp(-e)) / e.shape[0]
    return ious


def ground_truth_of(image, rows):
    """The image's objects `rows` as pycocotools holds them after _prepare."""
    out = []
    for g in rows:
        crowd = bool(image["gt_crowd"][g])
        out.append(dict(id=g + 1, area=float(image["gt_area"][g]), crowd=crowd,
                        ignore=crowd or int(image["gt_num_keypoints"][g]) == 0,
                        bbox=[float(v) for v in image["gt_boxes"][g]],
                        keypoints=np.asarray(image["gt_keypoints"][g], np.float64).flatten().tolist()))
    return out


def for_the_matcher(gts):
    """-> what coco_eval_ref.evaluate_image_category reads (id, area, crowd): see the module docstring."""
    return [dict(id=g["id"], crowd=g["crowd"], area=g["area"] if g["crowd"] or not g["ignore"] else -np.inf)
            for g in gts]


def evaluate_images(dataset, num_categories, sigmas):
    """coco_eval_ref.evaluate_images for the keypoints task: the same three results, `ious` holding the OKS rows."""
    order = sorted(range(len(dataset)), key=lambda j: dataset[j]["image_id"])
    evals, per_image = {}, []
    for i, j in enumerate(order):
        image = dataset[j]
        dets = detections_of(image)
        rank = np.full(len(dets), -1, np.int64)
        info = dict(rank=rank, ious={}, gt_rows={}, det_rows={})
        for c in range(num_categories):
            mine = [d for d in dets if d["cat"] == c]
            mine = [mine[k] for k in CR.stable_order([d["score"] for d in mine])][:MAX_DETS[-1]]
            for r, d in enumerate(mine):
                rank[d["row"]] = r
            rows = [g for g in range(len(image["gt_cats"])) if int(image["gt_cats"][g]) == c]
            gts = ground_truth_of(image, rows)
            ious = [[float(v) for v in row] for row in compute_oks(mine, gts, sigmas)]
            info["ious"][c], info["gt_rows"][c], info["det_rows"][c] = ious, rows, [d["row"] for d in mine]
            for a, rng in enumerate(AREA_RNG):
                m, ig, gig = CR.evaluate_image_category(mine, for_the_matcher(gts), ious, rng, IOU_THRS)
                evals[(i, c, a)] = dict(scores=[d["score"] for d in mine], matches=m, ignores=ig, gt_ignores=gig)
        per_image.append(info)
    return order, evals, per_image


def summarize(precision, recall):
    """pycocotools' _summarizeKps: ten stats, all at maxDets 20."""
    def one(ap, iou=None, area=0):
        s = precision[:, :, :, area, 0] if ap else recall[:, :, area, 0]
        if iou is not None:
            s = s[np.where(iou == IOU_THRS)[0]]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    return np.array([one(1), one(1, iou=.5), one(1, iou=.75), one(1, area=1), one(1, area=2),
                     one(0), one(0, iou=.5), one(0, iou=.75), one(0, area=1), one(0, area=2)], dtype=np.float64)


def derive_results(stats, precision, class_names=None):
    """_derive_coco_results (coco_evaluation.py:288-354) with the keypoints metrics (:305)."""
    if stats is None:
        return {metric: float("nan") for metric in METRICS}
    results = {metric: float(stats[idx] * 100 if stats[idx] >= 0 else "nan") for idx, metric in enumerate(METRICS)}
    if class_names is None or len(class_names) <= 1:
        return results
    for idx, name in enumerate(class_names):
        p = precision[:, :, idx, 0, -1]
        p = p[p > -1]
        results["AP-" + "{}".format(name)] = float((np.mean(p) if p.size else float("nan")) * 100)
    return results


def evaluate(dataset, num_categories, sigmas, class_names=None):
    """-> (the `keypoints` entry of COCOEvaluator.evaluate's result, dict(precision, scores (T,R,K,3,1), recall
    (T,K,3,1), npos (K,3), stats (10), order, evals, per_image))."""
    order, evals, per_image = evaluate_images(dataset, num_categories, sigmas)
    precision, scores, recall, npos = CR.accumulate(evals, len(dataset), num_categories, max_dets=MAX_DETS,
                                                    num_areas=len(AREA_RNG))
    stats = summarize(precision, recall)
    any_det = any(len(im["det_scores"]) for im in dataset)
    result = derive_results(stats if any_det else None, precision, class_names)
    return result, dict(precision=precision, scores=scores, recall=recall, npos=npos, stats=stats, order=order,
                        evals=evals, per_image=per_image)


def match_bits(evals, i, c, num_dets):
    """The device's record words: coco_eval_ref.match_bits over the task's three area ranges, and the bits of the
    device's spare fourth range, which repeats the third."""
    T, A = len(IOU_THRS), len(AREA_RNG)
    matched, ignore = CR.match_bits(evals, i, c, num_dets, num_areas=A)
    spare = lambda w: w | (((w >> ((A - 1) * T)) & ((1 << T) - 1)) << (A * T))  # noqa: E731
    return [spare(w) for w in matched], [spare(w) for w in ignore]


def margins(per_image, dataset, order):
    """The margin condition of the recorded cases -> (the least distance of an OKS from a threshold, the least distance
    between two OKS of one detection and category, bit-identical ground-truth objects counted once)."""
    to_thr, to_other = np.inf, np.inf
    for i, info in enumerate(per_image):
        image = dataset[order[i]]
        for c, rows in info["ious"].items():
            gt_rows = info["gt_rows"][c]
            key = [(image["gt_keypoints"][g].tobytes(), image["gt_boxes"][g].tobytes(), image["gt_area"][g].tobytes())
                   for g in gt_rows]
            first = [k for k in range(len(key)) if key[k] not in key[:k]]
            for row in rows:
                v = np.array(row, np.float64)
                assert all(v[k] == v[key.index(key[k])] for k in range(len(key)))
                v = v[first]
                to_thr = min(to_thr, float(np.abs(v[:, None] - IOU_THRS[None]).min())) if v.size else to_thr
                if v.size > 1:
                    to_other = min(to_other, float(np.diff(np.sort(v)).min()))
    return to_thr, to_other


# ---------------------------------------------------------------------------------------------- recorded cases
def dataset_to_fields(dataset, sigmas, processed):
    f = CR.dataset_to_fields(dataset)
    P = len(sigmas)
    cat = lambda key, dt: np.concatenate([np.asarray(im[key], dt).reshape(-1, P, 3) for im in dataset])  # noqa: E731
    f.update(det_keypoints=cat("det_keypoints", np.float32), gt_keypoints=cat("gt_keypoints", np.float64),
             gt_num_keypoints=np.concatenate([np.asarray(im["gt_num_keypoints"], np.int64) for im in dataset]),
             sigmas=np.asarray(sigmas, np.float64), processed=np.asarray(processed, bool))
    return f


def dataset_from_fields(f):
    """-> (dataset, sigmas, processed (N,) bool: an unprocessed image has no detections and is never shown to the
    evaluator)."""
    dataset = CR.dataset_from_fields(f)
    d0 = g0 = 0
    for i, im in enumerate(dataset):
        d1, g1 = d0 + int(f["det_count"][i]), g0 + int(f["gt_count"][i])
        im.update(det_keypoints=f["det_keypoints"][d0:d1], gt_keypoints=f["gt_keypoints"][g0:g1],
                  gt_num_keypoints=f["gt_num_keypoints"][g0:g1])
        d0, g0 = d1, g1
    return dataset, f["sigmas"], f["processed"]

