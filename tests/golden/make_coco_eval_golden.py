"""Records tests/golden/coco_eval_reference.npz — build container only.  It compiles the reference's own
detectron2/layers/csrc/cocoeval/cocoeval.cpp where it lies into a temporary directory, behind a small pybind binding
written here (InstanceAnnotation, ImageEvaluation's fields read-only, EvaluateImages, Accumulate); nothing of the
reference is copied and nothing compiled is kept.

    python tests/golden/make_coco_eval_golden.py

pycocotools is not installed, so the compiled code is fed what COCOeval_opt.evaluate would feed it, built by the
restatement (tests/coco_eval_ref.py): per (image in ascending id order, category) the ground-truth and detection
instances in annotation / Instances row order and the IoU rows of the score-sorted, truncated detections; the
parameters as a SimpleNamespace.  Recorded per case and task: the inputs, per (category, area range, image) the
detection_matches, detection_ignores and ground_truth_ignores of the compiled code, and its precision / scores /
recall tables.  The IoU itself is therefore the restatement's (DESIGN.md §4g says so); matching and accumulation are
the reference's.

The cases, asserted below: a crowd ground truth matched by two detections; a category without ground truth, with and
without detections; a category without detections; equal scores inside a category within one image and across
images; two ground-truth boxes with identical IoU to one detection; objects on both sides of 32^2 and 96^2; more than
100 detections of one category in one image; image ids that are not in process() order."""
import importlib.util
import os
import subprocess
import sys
import sysconfig
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import coco_eval_ref as CR  # noqa: E402

REF_DIR = "/root/reference/detectron2/layers/csrc/cocoeval"
OUT = os.path.join(HERE, "coco_eval_reference.npz")
K = 6

BINDING = r"""
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>
#include "cocoeval.h"
namespace py = pybind11;
using namespace detectron2::COCOeval;
PYBIND11_MODULE(coco_ref_binding, m) {
  py::class_<InstanceAnnotation>(m, "InstanceAnnotation").def(py::init<uint64_t, double, double, bool, bool>());
  py::class_<ImageEvaluation>(m, "ImageEvaluation")
      .def_readonly("detection_matches", &ImageEvaluation::detection_matches)
      .def_readonly("detection_scores", &ImageEvaluation::detection_scores)
      .def_readonly("ground_truth_ignores", &ImageEvaluation::ground_truth_ignores)
      .def_readonly("detection_ignores", &ImageEvaluation::detection_ignores);
  m.def("EvaluateImages", &EvaluateImages);
  m.def("Accumulate", &Accumulate);
}
"""


def compiled_reference(tmp):
    import pybind11

    src = os.path.join(tmp, "binding.cpp")
    with open(src, "w") as f:
        f.write(BINDING)
    so = os.path.join(tmp, "coco_ref_binding" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", REF_DIR, "-I", pybind11.get_include(),
                           "-I", sysconfig.get_paths()["include"], src, os.path.join(REF_DIR, "cocoeval.cpp"), "-o", so])
    spec = importlib.util.spec_from_file_location("coco_ref_binding", so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def shape_mask(rng, H, W, box):
    """A filled ellipse or rectangle inside the XYWH box."""
    x, y, w, h = box
    yy, xx = np.mgrid[0:H, 0:W]
    if rng.random() < 0.5:
        return (xx >= x) & (xx < x + w) & (yy >= y) & (yy < y + h)
    cx, cy = x + w / 2.0, y + h / 2.0
    return ((xx + 0.5 - cx) / (w / 2.0)) ** 2 + ((yy + 0.5 - cy) / (h / 2.0)) ** 2 <= 1.0


def make_case(seed, N, masks, crowded_image):
    """Categories: 0, 1, 2, 5 have ground truth and detections; 3 never has ground truth (detections in odd seeds);
    4 has ground truth and never a detection.  Scores lie on a grid of twentieths: plenty of ties."""
    rng = np.random.default_rng(seed)
    H, W = (101, 119) if masks else (240, 320)
    ids = (rng.permutation(N) * 7 + 3).tolist()                          # not in ascending order
    dataset = []
    for i in range(N):
        gt_cats, gt_boxes, gt_crowd = [], [], []
        for _ in range(int(rng.integers(0, 6)) if i != 1 else 0):        # image 1: no ground truth
            side = [rng.uniform(6, 30), rng.uniform(34, 90), rng.uniform(97, min(H, W) - 2)][int(rng.integers(3))]
            w, h = side * rng.uniform(0.8, 1.0), side * rng.uniform(1.0, 1.2)
            w, h = min(w, W - 1), min(h, H - 1)
            x, y = rng.uniform(0, W - w), rng.uniform(0, H - h)
            gt_cats.append(int(rng.choice([0, 1, 2, 4, 5])))
            gt_boxes.append([float(np.round(v, 2)) for v in (x, y, w, h)])
            gt_crowd.append(int(rng.random() < 0.15))
        if i == 0:                                                       # a crowd region and two identical boxes
            gt_cats += [0, 1, 1]
            gt_boxes += [[10.0, 12.0, 60.0, 50.0], [30.0, 30.0, 40.0, 36.0], [30.0, 30.0, 40.0, 36.0]]
            gt_crowd += [1, 0, 0]
        gt_masks = np.stack([shape_mask(rng, H, W, b) for b in gt_boxes]) if gt_boxes else np.zeros((0, H, W), bool)
        gt_area = [float(m.sum()) for m in gt_masks] if masks else [b[2] * b[3] * 0.75 for b in gt_boxes]
        boxes, scores, classes = [], [], []

        def det(b, c, s=None):
            boxes.append([b[0], b[1], b[0] + b[2], b[1] + b[3]])
            classes.append(c)
            scores.append(float(rng.integers(1, 20)) / 20.0 if s is None else s)

        for b, c in zip(gt_boxes, gt_cats):
            if c == 4:
                continue
            for _ in range(int(rng.integers(0, 3))):
                j = rng.normal(0, 0.08, 4) * np.array([b[2], b[3], b[2], b[3]])
                det([b[0] + j[0], b[1] + j[1], max(b[2] + j[2], 1.0), max(b[3] + j[3], 1.0)],
                    c if rng.random() < 0.9 else int(rng.choice([0, 1, 2, 5])))
        for _ in range(int(rng.integers(0, 4)) if i != 2 else 0):        # image 2: no detections
            w, h = rng.uniform(5, W / 2), rng.uniform(5, H / 2)
            det([rng.uniform(0, W - w), rng.uniform(0, H - h), w, h], int(rng.choice([0, 1, 2, 5])))
        if seed % 2 == 1:
            det([5.0, 5.0, 30.0, 30.0], 3)
        if i == 0:
            det([12.0, 14.0, 30.0, 30.0], 0, 0.9)                         # two detections inside the crowd region
            det([20.0, 16.0, 40.0, 40.0], 0, 0.9)
            det([30.0, 30.0, 40.0, 36.0], 1, 0.7)                         # the same IoU with both identical boxes
        if i == crowded_image:
            for k in range(105):                                         # more than max_det of one category
                det([40.0 + (k % 15) * 3, 30.0 + (k // 15) * 4, 50.0, 45.0], 0, float(1 + k % 19) / 20.0)
        order = rng.permutation(len(boxes))
        boxes = np.array(boxes, np.float32).reshape(-1, 4)[order]
        det_masks = None
        if masks:
            det_masks = np.stack([shape_mask(rng, H, W, [b[0], b[1], b[2] - b[0], b[3] - b[1]]) for b in boxes]) \
                if len(boxes) else np.zeros((0, H, W), bool)
        dataset.append(dict(
            image_id=ids[i], det_boxes=boxes, det_scores=np.array(scores, np.float32)[order],
            det_classes=np.array(classes, np.int64)[order], det_masks=det_masks,
            gt_cats=np.array(gt_cats, np.int64), gt_boxes=np.array(gt_boxes, np.float64).reshape(-1, 4),
            gt_area=np.array(gt_area, np.float64), gt_crowd=np.array(gt_crowd, np.uint8),
            gt_masks=gt_masks if masks else None))
    return dataset


def run_reference(mod, dataset, task):
    """-> what the compiled code says, in the layout of CR.flatten_evals / CR.accumulate."""
    order, _, per_image = CR.evaluate_images(dataset, task, K)
    gts, dts, ious = [], [], []
    for i, j in enumerate(order):
        image = dataset[j]
        dets = CR.detections_of(image, task)
        g_row, d_row, i_row = [], [], []
        for c in range(K):
            rows = [g for g in range(len(image["gt_cats"])) if int(image["gt_cats"][g]) == c]
            g_row.append([mod.InstanceAnnotation(g + 1, 0.0, float(image["gt_area"][g]), bool(image["gt_crowd"][g]),
                                                 bool(image["gt_crowd"][g])) for g in rows])
            d_row.append([mod.InstanceAnnotation(d["row"] + 1, d["score"], d["area"], False, False)
                          for d in dets if d["cat"] == c])
            i_row.append(per_image[i]["ious"][c])
        gts.append(g_row)
        dts.append(d_row)
        ious.append(i_row)
    params = types.SimpleNamespace(
        recThrs=[float(v) for v in CR.REC_THRS], maxDets=list(CR.MAX_DETS), iouThrs=[float(v) for v in CR.IOU_THRS],
        useCats=1, catIds=list(range(K)), areaRng=[[float(v) for v in r] for r in CR.AREA_RNG],
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


def check_conditions(dataset, ref_bbox):
    ids = [im["image_id"] for im in dataset]
    assert ids != sorted(ids)
    dcls = np.concatenate([im["det_classes"] for im in dataset])
    gcls = np.concatenate([im["gt_cats"] for im in dataset])
    assert (gcls == 3).sum() == 0 and (dcls == 4).sum() == 0 and (gcls == 4).sum() > 0
    area = np.concatenate([im["gt_area"] for im in dataset])
    assert (area < 32 ** 2).any() and ((area > 32 ** 2) & (area < 96 ** 2)).any()
    assert dataset[0]["det_masks"] is not None or (area > 96 ** 2).any()     # (the mask cases' images are 101 x 119)
    within = across = False
    seen = {}
    for i, im in enumerate(dataset):
        for c in range(K):
            s = im["det_scores"][im["det_classes"] == c].tolist()
            within |= len(set(s)) < len(s)
            across |= any(v in seen.get(c, set()) for v in s)
        for c in range(K):
            seen.setdefault(c, set()).update(im["det_scores"][im["det_classes"] == c].tolist())
    assert within and across


def main():
    cases = OrderedDict_cases()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        mod = compiled_reference(tmp)
        for name, (seed, N, masks, crowded) in cases.items():
            dataset = make_case(seed, N, masks, crowded)
            for k, v in CR.dataset_to_fields(dataset).items():
                out["%s__%s" % (name, k)] = v
            for task in (("bbox", "segm") if masks else ("bbox",)):
                ref = run_reference(mod, dataset, task)
                if task == "bbox":
                    check_conditions(dataset, ref)
                for k, v in ref.items():
                    out["%s__%s_%s" % (name, task, k)] = v
                print(name, task, "evals", len(ref["sizes"]), "AP", CR.summarize(ref["precision"], ref["recall"])[0])
    facts = case_facts(out, cases)
    assert facts["crowd_twice"] and facts["over_100"] and facts["cat3_with"] and facts["cat3_without"], facts
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


def OrderedDict_cases():
    from collections import OrderedDict

    # name -> (seed, images, masks, index of the image with 105 detections of category 0 or -1)
    return OrderedDict([("a", (10, 8, True, -1)), ("b", (11, 7, True, -1)), ("c", (12, 14, False, 3)),
                        ("d", (13, 12, False, 5))])


def case_facts(out, cases):
    """Properties that need the recorded matches: the crowd region of image 0 matched by two detections; more than 100
    detections of a category in an image (its evaluation keeps 100); category 3 with and without detections."""
    facts = dict(crowd_twice=False, over_100=False, cat3_with=False, cat3_without=False)
    for name, (seed, N, masks, crowded) in cases.items():
        dataset = CR.dataset_from_fields({k.split("__")[1]: v for k, v in out.items() if k.startswith(name + "__")})
        n3 = sum(int((im["det_classes"] == 3).sum()) for im in dataset)
        facts["cat3_with"] |= n3 > 0
        facts["cat3_without"] |= n3 == 0
        facts["over_100"] |= any(int((im["det_classes"] == 0).sum()) > 100 for im in dataset)
        order = sorted(range(N), key=lambda j: dataset[j]["image_id"])
        i0 = order.index(0)
        sizes, matches = out[name + "__bbox_sizes"], out[name + "__bbox_matches"]
        T = len(CR.IOU_THRS)
        starts = np.concatenate([[0], np.cumsum(sizes[:, 0] * T)])
        e = (0 * len(CR.AREA_RNG) + 0) * N + i0                          # category 0, all areas, image 0
        m = matches[starts[e]:starts[e + 1]].reshape(T, -1)[0]
        crowd_row = int(np.flatnonzero((dataset[0]["gt_cats"] == 0) & (dataset[0]["gt_crowd"] == 1)
                                       & (dataset[0]["gt_boxes"][:, 2] == 60.0))[0])
        facts["crowd_twice"] |= int((m == crowd_row + 1).sum()) >= 2
    return facts


if __name__ == "__main__":
    main()
