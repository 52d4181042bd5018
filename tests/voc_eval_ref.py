"""NumPy restatement of the reference's Pascal VOC evaluation over arrays — the yardstick of the device evaluator
(jtsm_amd/csrc/voc_eval.hip).  Restated from detectron2/evaluation/pascal_voc_evaluation.py: process() :55-69 (what is
printed), voc_eval :242-355, voc_ap :210-239, voc_eval_corloc :358-452; nothing of it is copied.

The detections really go through text: every score is formatted with ".3f" and every coordinate with ".1f" (xmin and
ymin after `+ 1` in float32, as NumPy scalar arithmetic does it there) and parsed back with float(), so the device's
integer quantisation is checked against Python's formatting.  The one declared difference from the reference: the
ranking is `np.argsort(-confidence, kind="stable")` — descending quantised score, equal scores in arrival order — where
the reference's plain argsort leaves the order among equal scores to NumPy's introsort.

Ground truth comes as the evaluator keeps it: gt_boxes (G,4) int (VOC 1-based, as in the XML), gt_difficult (G),
sorted by (class, image), and gt_offsets (C*N+1), the CSR over (class, image), class-major."""
import numpy as np

THRESHOLDS = [t / 100.0 for t in range(50, 100, 5)]


def through_text(boxes, scores):
    """-> (confidence (D,) float64, BB (D,4) float64): the numbers voc_eval parses out of the file process() wrote."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    scores = np.asarray(scores, np.float32)
    conf = np.empty(len(scores), np.float64)
    bb = np.empty((len(scores), 4), np.float64)
    one = np.float32(1)
    for d in range(len(scores)):
        xmin, ymin, xmax, ymax = boxes[d]
        xmin = np.float32(xmin + one)
        ymin = np.float32(ymin + one)
        line = f"{float(scores[d]):.3f} {float(xmin):.1f} {float(ymin):.1f} {float(xmax):.1f} {float(ymax):.1f}"
        v = [float(z) for z in line.split(" ")]
        conf[d] = v[0]
        bb[d] = v[1:]
    return conf, bb


def _overlaps(bb, bbgt):
    ixmin = np.maximum(bbgt[:, 0], bb[0])
    iymin = np.maximum(bbgt[:, 1], bb[1])
    ixmax = np.minimum(bbgt[:, 2], bb[2])
    iymax = np.minimum(bbgt[:, 3], bb[3])
    iw = np.maximum(ixmax - ixmin + 1.0, 0.0)
    ih = np.maximum(iymax - iymin + 1.0, 0.0)
    inters = iw * ih
    uni = ((bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0)
           + (bbgt[:, 2] - bbgt[:, 0] + 1.0) * (bbgt[:, 3] - bbgt[:, 1] + 1.0) - inters)
    return inters / uni


def voc_ap(rec, prec, use_07_metric):
    if use_07_metric:
        ap = 0.0
        for t in np.arange(0.0, 1.1, 0.1):
            sel = rec >= t
            p = np.max(prec[sel]) if np.sum(sel) != 0 else 0
            ap = ap + p / 11.0
        return ap
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def evaluate(boxes, scores, classes, images, gt_boxes, gt_difficult, gt_offsets, N, C, use_07_metric,
             keep_curves=False):
    """-> dict: order / tp_bits / fp_bits (D,) in input order, counts (C,2) = [npos, npos_im], ap / corloc (10,C)
    float64 fractions, and with keep_curves rec / prec as {(t, c): array}."""
    classes = np.asarray(classes).astype(np.int64)
    images = np.asarray(images).astype(np.int64)
    gt_boxes = np.asarray(gt_boxes).reshape(-1, 4)
    gt_difficult = np.asarray(gt_difficult).astype(bool)
    D = len(classes)
    conf, BB = through_text(boxes, scores)
    order = np.full(D, -1, np.int32)
    tp_bits, fp_bits = np.zeros(D, np.uint16), np.zeros(D, np.uint16)
    counts = np.zeros((C, 2), np.int32)
    ap, corloc = np.zeros((10, C)), np.zeros((10, C))
    curves = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in range(C):
            lo = gt_offsets[c * N:(c + 1) * N + 1]
            npos = int(np.sum(~gt_difficult[lo[0]:lo[-1]]))
            npos_im = sum(1 for i in range(N) if np.any(~gt_difficult[lo[i]:lo[i + 1]]))
            counts[c] = npos, npos_im
            idx = np.nonzero(classes == c)[0]                    # arrival order
            sorted_ind = idx[np.argsort(-conf[idx], kind="stable")]
            nd = len(sorted_ind)
            order[sorted_ind] = np.arange(nd)
            # the overlaps do not depend on the threshold: once per detection
            ovmax, jmax = np.full(nd, -np.inf), np.zeros(nd, np.int64)
            # CorLoc looks at an image's highest-ranked detection only, and only in images with a non-difficult box
            first, seen = np.zeros(nd, bool), set()
            for d, e in enumerate(sorted_ind):
                im = images[e]
                a, b = lo[im], lo[im + 1]
                if b > a:
                    ov = _overlaps(BB[e], gt_boxes[a:b].astype(float))
                    ovmax[d], jmax[d] = np.max(ov), np.argmax(ov)
                if im not in seen and np.any(~gt_difficult[a:b]):
                    seen.add(im)
                    first[d] = True
            for t, thr in enumerate(THRESHOLDS):
                claimed = np.zeros(len(gt_difficult), bool)
                tp, fp = np.zeros(nd), np.zeros(nd)
                hits = int(np.sum(ovmax[first] > thr))
                for d, e in enumerate(sorted_ind):
                    a = lo[images[e]]
                    if ovmax[d] > thr:
                        j = a + jmax[d]
                        if not gt_difficult[j]:
                            if not claimed[j]:
                                tp[d] = 1.0
                                claimed[j] = True
                            else:
                                fp[d] = 1.0
                    else:
                        fp[d] = 1.0
                tp_bits[sorted_ind] |= (tp.astype(np.uint16) << t).astype(np.uint16)
                fp_bits[sorted_ind] |= (fp.astype(np.uint16) << t).astype(np.uint16)
                fpc, tpc = np.cumsum(fp), np.cumsum(tp)
                rec = tpc / float(npos)
                prec = tpc / np.maximum(tpc + fpc, np.finfo(np.float64).eps)
                ap[t, c] = voc_ap(rec, prec, use_07_metric)
                corloc[t, c] = 0.0 if nd == 0 else (np.nan if npos_im == 0 else 1.0 * hits / npos_im)
                if keep_curves:
                    curves[(t, c)] = (rec, prec)
    out = dict(order=order, tp_bits=tp_bits, fp_bits=fp_bits, counts=counts, ap=ap, corloc=corloc)
    if keep_curves:
        out["curves"] = curves
    return out


def result_dict(ap, corloc):
    """The reference's dictionary from the (10, C) tables: per threshold the mean over classes of x100 values."""
    m_ap = [np.mean([v * 100 for v in row]) for row in ap]
    m_cl = [np.mean([v * 100 for v in row]) for row in corloc]
    return {"bbox": {"AP": np.mean(m_ap), "AP50": m_ap[0], "AP75": m_ap[5]},
            "bbox CorLoc": {"CL": np.mean(m_cl), "CL50": m_cl[0], "CL75": m_cl[5]}}


def csr_from_objects(objects, N, C):
    """objects: rows (image, class, difficult, xmin, ymin, xmax, ymax) in file order -> (gt_boxes, gt_difficult,
    gt_offsets) sorted by (class, image), file order inside."""
    o = np.asarray(objects, np.int64).reshape(-1, 7)
    key = o[:, 1] * N + o[:, 0]
    perm = np.argsort(key, kind="stable")
    o, key = o[perm], key[perm]
    offsets = np.zeros(C * N + 1, np.int32)
    np.cumsum(np.bincount(key, minlength=C * N), out=offsets[1:])
    return o[:, 3:7].astype(np.int32), o[:, 2].astype(np.uint8), offsets
