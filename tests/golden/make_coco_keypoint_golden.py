"""Records tests/golden/coco_keypoint_reference.npz — build container only.  As make_coco_eval_golden.py (whose
compiled_reference() it uses): the reference's own detectron2/layers/csrc/cocoeval/cocoeval.cpp is compiled where it
lies into a temporary directory behind a small binding written there; nothing of the reference is copied and nothing
compiled is kept.

    python tests/golden/make_coco_keypoint_golden.py

The compiled code is fed what COCOeval_opt.evaluate would feed it for the keypoints task, built by the restatement
(tests/coco_keypoint_ref.py): per (image in ascending id order, category) the ground-truth instances with their
SEPARATE is_crowd and ignore flags (ignore := iscrowd or num_keypoints == 0), the detection instances and the OKS rows
of the score-sorted detections cut at 20; the keypoints parameters (maxDets [20], three area ranges).  Recorded per
case: the inputs, per (category, area range, image) the detection_matches, detection_ignores and
ground_truth_ignores of the compiled code, and its precision / scores / recall tables.  So OKS is the restatement's;
matching and accumulation are the reference's.

Two cases of four images: `p5` with five keypoints and custom sigmas, `p17` with the 17 COCO sigmas.  Asserted below
for each: more than 20 detections of one category in one image; a crowd object matched by two detections; an object
with num_keypoints == 0 that is no crowd and the best match of two detections (the first is matched and ignored, the
second is not matched to it again — a matcher with one flag for both would); that object has all v == 0, so its OKS is
the box-distance branch, with detections inside (OKS exactly 1) and outside its doubled box; a detection equal to a
ground truth after the 0.5 shift (OKS exactly 1); objects on both sides of 32^2 and 96^2; a category without ground
truth and one without detections; an unprocessed image; equal scores within and across images; two bit-identical
objects (the later one takes the tie); 66 objects of one category in one image; and the margin condition: every OKS at
least 1e-9 from each threshold and from every other OKS of its detection and category (bit-identical objects excepted).
All objects of an (image, category) lie within a few `s` of one pose, s = sqrt(2 (2 sigma_max)^2 600) pixels, so that no
two OKS of a detection sink towards zero together."""
import os
import sys
import tempfile
import types
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import coco_eval_ref as CR  # noqa: E402
import coco_keypoint_ref as KR  # noqa: E402
from make_coco_eval_golden import compiled_reference  # noqa: E402

OUT = os.path.join(HERE, "coco_keypoint_reference.npz")
K = 4                      # 0, 1: ground truth and detections; 2: ground truth only; 3: detections only
AREA_MIN = 600.0
CASES = OrderedDict([("p5", (21, np.array([0.05, 0.08, 0.1, 0.07, 0.12]))), ("p17", (22, KR.COCO_SIGMAS))])
# per image and category 0, 1, 2: ground-truth objects; per image and category 0, 1, 3: detections
GT_COUNTS = [[6, 3, 2], [66, 2, 1], [5, 2, 0], [3, 1, 0]]
DET_COUNTS = [[24, 4, 1], [12, 3, 0], [10, 5, 1], [0, 0, 0]]


def make_case(seed, sigmas):
    rng = np.random.default_rng(seed)
    P = len(sigmas)
    s = float(np.sqrt(2 * (2 * sigmas.max()) ** 2 * AREA_MIN))
    ids = [31, 5, 17, 11]
    dataset, facts = [], {}
    for i in range(4):
        gt = dict(cats=[], boxes=[], area=[], crowd=[], kp=[], nk=[])
        dets = dict(boxes=[], scores=[], classes=[], kp=[])

        def add_gt(c, kp, area=None, crowd=0, box=None):
            kp = np.asarray(kp, np.float64)
            if area is None:
                area = float(rng.choice([rng.uniform(AREA_MIN, 1000), rng.uniform(1100, 9000), rng.uniform(9300, 12000)]))
            if box is None:
                lo, hi = kp[:, :2].min(0) - 2, kp[:, :2].max(0) + 2
                box = [lo[0], lo[1], hi[0] - lo[0], hi[1] - lo[1]]
            gt["cats"].append(c)
            gt["boxes"].append([float(v) for v in box])
            gt["area"].append(float(area))
            gt["crowd"].append(crowd)
            gt["kp"].append(kp)
            gt["nk"].append(int((kp[:, 2] > 0).sum()))
            return len(gt["cats"]) - 1

        def add_det(c, xy, score=None):
            """xy: the (P, 2) points as the evaluation is to see them (the model's output lies 0.5 above)."""
            kp = np.concatenate([np.asarray(xy) + 0.5, rng.uniform(0.05, 1, (P, 1))], 1).astype(np.float32)
            side = float(np.sqrt(rng.choice([rng.uniform(300, 900), rng.uniform(1200, 8000), rng.uniform(9500, 20000)])))
            x0, y0 = kp[:, 0].min() - 1, kp[:, 1].min() - 1
            dets["boxes"].append([x0, y0, x0 + side * rng.uniform(0.8, 1.2), y0 + side])
            dets["classes"].append(c)
            dets["scores"].append(float(rng.integers(1, 20)) / 20.0 if score is None else score)
            dets["kp"].append(kp)
            return len(dets["classes"]) - 1

        def near(xy, sd):
            return xy + np.clip(rng.normal(0, sd * s, (P, 2)), -0.4 * s, 0.4 * s)

        for c in range(3):
            base = rng.uniform(40, 200, (P, 2))
            mine = []
            for k in range(GT_COUNTS[i][c]):
                xy = base + rng.uniform(-0.5, 0.5, 2) * s + rng.uniform(-0.15, 0.15, (P, 2)) * s
                v = rng.choice([0.0, 1.0, 2.0], P, p=[0.2, 0.3, 0.5])
                v[int(rng.integers(P))] = 2.0
                kp = np.concatenate([xy, v[:, None]], 1)
                if c == 0 and k == 0 and i == 0:                          # a crowd region with keypoints of its own
                    facts["crowd"] = (i, add_gt(c, kp, crowd=1))
                elif c == 0 and k == 1 and i == 0:                        # quarter pixels: + 0.5 is exact in fp32
                    kp[:, :2] = np.round(kp[:, :2] * 4) / 4
                    facts["exact_gt"] = (i, add_gt(c, kp))
                elif c == 1 and k == 0 and i in (0, 2):                   # no labelled keypoint, no crowd
                    kp[:, 2] = 0.0
                    X0, X1 = base.min(0) - 0.3 * s, base.max(0) + 0.3 * s   # the doubled box, a little inside the spread
                    w = (X1 - X0) / 3
                    g = add_gt(c, kp, area=2500.0, box=[X0[0] + w[0], X0[1] + w[1], w[0], w[1]])
                    if i == 0:
                        facts["unlabelled"] = (i, g, X0, X1)
                elif c == 0 and k == 1 and i == 2:                        # two bit-identical objects
                    first = add_gt(c, kp, area=3000.0)
                    facts["twins"] = (i, first, add_gt(c, kp, area=3000.0))
                    mine.append(first)
                    continue
                else:
                    add_gt(c, kp)
                mine.append(len(gt["cats"]) - 1)
            if c == 2:
                continue
            n = DET_COUNTS[i][c]
            made = 0
            if c == 0 and i == 0:
                g = facts["crowd"][1]
                add_det(0, near(gt["kp"][g][:, :2], 0.02), 0.9)          # two detections on the crowd region
                add_det(0, near(gt["kp"][g][:, :2], 0.02), 0.85)
                facts["exact_det"] = add_det(0, gt["kp"][facts["exact_gt"][1]][:, :2], 0.7)
                made = 3
            if c == 0 and i == 2:
                add_det(0, near(gt["kp"][facts["twins"][1]][:, :2], 0.03), 0.95)
                made = 1
            if c == 1 and i == 0:
                _, g, X0, X1 = facts["unlabelled"]
                inside = lambda xy: np.clip(xy, X0 + 1, X1 - 1)  # noqa: E731
                facts["inside"] = [add_det(1, inside(near(gt["kp"][g][:, :2], 0.3)), 0.99),
                                   add_det(1, inside(near(gt["kp"][g][:, :2], 0.3)), 0.97)]
                xy = near(gt["kp"][g][:, :2], 0.2)
                xy[0] = X0 - 0.6 * s                                     # one point outside the doubled box
                facts["outside"] = add_det(1, xy, 0.5)
                made = 3
            for _ in range(n - made):
                g = mine[int(rng.integers(len(mine)))]
                add_det(c, near(gt["kp"][g][:, :2], float(rng.choice([0.05, 0.12, 0.25]))))
        for _ in range(DET_COUNTS[i][2]):                                # category 3: detections without ground truth
            add_det(3, rng.uniform(40, 200, (P, 2)))
        order = rng.permutation(len(dets["classes"]))
        facts.setdefault("det_rows", {})[i] = np.argsort(order)          # detection as added -> its row
        G = len(gt["cats"])
        dataset.append(dict(
            image_id=ids[i], det_boxes=np.array(dets["boxes"], np.float32).reshape(-1, 4)[order],
            det_scores=np.array(dets["scores"], np.float32)[order], det_classes=np.array(dets["classes"], np.int64)[order],
            det_masks=None, det_keypoints=np.array(dets["kp"], np.float32).reshape(-1, P, 3)[order],
            gt_cats=np.array(gt["cats"], np.int64), gt_boxes=np.array(gt["boxes"], np.float64).reshape(G, 4),
            gt_area=np.array(gt["area"], np.float64), gt_crowd=np.array(gt["crowd"], np.uint8), gt_masks=None,
            gt_keypoints=np.array(gt["kp"], np.float64).reshape(G, P, 3), gt_num_keypoints=np.array(gt["nk"], np.int64)))
    return dataset, [True, True, True, False], facts


def run_reference(mod, dataset, sigmas):
    """-> what the compiled code says, in the layout of CR.flatten_evals / CR.accumulate."""
    order, _, per_image = KR.evaluate_images(dataset, K, sigmas)
    gts, dts, ious = [], [], []
    for i, j in enumerate(order):
        image = dataset[j]
        dets = KR.detections_of(image)
        g_row, d_row, i_row = [], [], []
        for c in range(K):
            rows = [g for g in range(len(image["gt_cats"])) if int(image["gt_cats"][g]) == c]
            g_row.append([mod.InstanceAnnotation(g["id"], 0.0, g["area"], g["crowd"], g["ignore"])
                          for g in KR.ground_truth_of(image, rows)])
            d_row.append([mod.InstanceAnnotation(d["row"] + 1, d["score"], d["area"], False, False)
                          for d in dets if d["cat"] == c])
            i_row.append(per_image[i]["ious"][c])
        gts.append(g_row)
        dts.append(d_row)
        ious.append(i_row)
    params = types.SimpleNamespace(
        recThrs=[float(v) for v in KR.REC_THRS], maxDets=list(KR.MAX_DETS), iouThrs=[float(v) for v in KR.IOU_THRS],
        useCats=1, catIds=list(range(K)), areaRng=[[float(v) for v in r] for r in KR.AREA_RNG],
        imgIds=[dataset[j]["image_id"] for j in order])
    evals = mod.EvaluateImages(params.areaRng, params.maxDets[-1], params.iouThrs, ious, gts, dts)
    acc = mod.Accumulate(params, evals)
    sizes, matches, ignores, gt_ignores = [], [], [], []
    for e in evals:                                                      # (category, area range, image) order
        sizes.append([len(e.detection_scores), len(e.ground_truth_ignores)])
        matches += list(e.detection_matches)
        ignores += list(e.detection_ignores)
        gt_ignores += list(e.ground_truth_ignores)
    counts = list(acc["counts"])
    return dict(sizes=np.array(sizes, np.int64).reshape(-1, 2), matches=np.array(matches, np.int64),
                ignores=np.array(ignores, bool), gt_ignores=np.array(gt_ignores, bool),
                precision=np.array(acc["precision"], np.float64).reshape(counts),
                scores=np.array(acc["scores"], np.float64).reshape(counts),
                recall=np.array(acc["recall"], np.float64).reshape(counts[:1] + counts[2:]))


def recorded_matches(ref, N, i, c, a=0):
    """(T, D) match ids of (image position i, category c, area range a) from the flat record."""
    T, A = len(KR.IOU_THRS), len(KR.AREA_RNG)
    starts = np.concatenate([[0], np.cumsum(ref["sizes"][:, 0] * T)])
    e = (c * A + a) * N + i
    return ref["matches"][starts[e]:starts[e + 1]].reshape(T, -1), ref["ignores"][starts[e]:starts[e + 1]].reshape(T, -1)


def check_conditions(dataset, processed, sigmas, facts, ref):
    N, T = len(dataset), len(KR.IOU_THRS)
    order, evals, per_image = KR.evaluate_images(dataset, K, sigmas)
    pos = {j: i for i, j in enumerate(order)}
    ids = [im["image_id"] for im in dataset]
    assert ids != sorted(ids) and 3 <= N <= 5
    assert all(len(im["det_scores"]) <= 30 and len(im["gt_cats"]) <= 70 for im in dataset)
    assert any(int((im["det_classes"] == 0).sum()) > 20 for im in dataset)
    assert any(int((im["gt_cats"] == 0).sum()) > 64 for im in dataset)
    dcls, gcls = (np.concatenate([im[k] for im in dataset]) for k in ("det_classes", "gt_cats"))
    assert (gcls == 3).sum() == 0 and (dcls == 3).sum() > 0 and (dcls == 2).sum() == 0 and (gcls == 2).sum() > 0
    area = np.concatenate([im["gt_area"] for im in dataset])
    assert (area < 32 ** 2).any() and ((area > 32 ** 2) & (area < 96 ** 2)).any() and (area > 96 ** 2).any()
    assert not processed[3] and len(dataset[3]["det_scores"]) == 0 and len(dataset[3]["gt_cats"]) > 0
    within = across = False
    seen = {}
    for im in dataset:
        for c in range(K):
            sc = im["det_scores"][im["det_classes"] == c].tolist()
            within |= len(set(sc)) < len(sc)
            across |= any(v in seen.get(c, set()) for v in sc)
        for c in range(K):
            seen.setdefault(c, set()).update(im["det_scores"][im["det_classes"] == c].tolist())
    assert within and across

    def oks_of(j, det_added, g):
        """OKS of the detection added as number det_added to image j with the image's object g, its rank, its row."""
        info = per_image[pos[j]]
        row = int(facts["det_rows"][j][det_added])
        c = int(dataset[j]["det_classes"][row])
        r = int(info["rank"][row])
        assert r >= 0
        return info["ious"][c][r][info["gt_rows"][c].index(g)], r, c

    # the crowd region is matched by two detections at one threshold
    j, g = facts["crowd"]
    m, _ = recorded_matches(ref, N, pos[j], 0)
    assert max(int((m[t] == g + 1).sum()) for t in range(T)) >= 2
    # a detection equal to a ground truth after the shift
    assert oks_of(0, facts["exact_det"], facts["exact_gt"][1])[0] == 1.0
    # the unlabelled object: OKS through the box distance, exactly 1 inside the doubled box, below 1 outside
    j, g, _, _ = facts["unlabelled"]
    im = dataset[j]
    assert im["gt_num_keypoints"][g] == 0 and not im["gt_crowd"][g] and not (im["gt_keypoints"][g][:, 2] > 0).any()
    (o1, r1, c), (o2, r2, _) = (oks_of(j, d, g) for d in facts["inside"])
    assert o1 == 1.0 and o2 == 1.0 and r1 < r2 and 0.5 < oks_of(j, facts["outside"], g)[0] < 1.0
    # ... the first detection is matched to it and ignored, the second is left unmatched at some threshold, although
    # the object is its best match there: a matcher that lets every ignored object match again decides otherwise
    m, ig = recorded_matches(ref, N, pos[j], c)
    ts = [t for t in range(T) if m[t][r1] == g + 1 and ig[t][r1] and m[t][r2] == 0 and not ig[t][r2]]
    assert ts, (m[:, r1], m[:, r2])
    info = per_image[pos[j]]
    rows = info["gt_rows"][c]
    merged = [dict(id=x["id"], area=x["area"], crowd=x["ignore"]) for x in KR.ground_truth_of(im, rows)]
    dets = [d for d in KR.detections_of(im) if d["cat"] == c]
    dets = [dets[k] for k in CR.stable_order([d["score"] for d in dets])][:20]
    m1, _, _ = CR.evaluate_image_category(dets, merged, info["ious"][c], KR.AREA_RNG[0], KR.IOU_THRS)
    assert all(m1[t][r2] == g + 1 for t in ts)
    # the bit-identical objects: the later one takes the tie
    j, first, second = facts["twins"]
    m, _ = recorded_matches(ref, N, pos[j], 0)
    r = oks_of(j, 0, first)[1]
    row = per_image[pos[j]]["ious"][0][r]
    k1, k2 = (per_image[pos[j]]["gt_rows"][0].index(g) for g in (first, second))
    assert row[k1] == row[k2] == max(row) and m[0][r] == second + 1
    # the margin condition
    to_thr, to_other = KR.margins(per_image, dataset, order)
    assert to_thr >= KR.MARGIN and to_other >= KR.MARGIN, (to_thr, to_other)
    return to_thr, to_other


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        mod = compiled_reference(tmp)
        for name, (seed, sigmas) in CASES.items():
            dataset, processed, facts = make_case(seed, sigmas)
            ref = run_reference(mod, dataset, sigmas)
            to_thr, to_other = check_conditions(dataset, processed, sigmas, facts, ref)
            for k, v in KR.dataset_to_fields(dataset, sigmas, processed).items():
                out["%s__%s" % (name, k)] = v
            for k, v in ref.items():
                out["%s__kp_%s" % (name, k)] = v
            print(name, "evals", len(ref["sizes"]), "AP", KR.summarize(ref["precision"], ref["recall"])[0],
                  "least distance of an OKS from a threshold %.3g, from another %.3g" % (to_thr, to_other))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
