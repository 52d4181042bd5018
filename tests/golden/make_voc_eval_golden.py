"""Records tests/golden/voc_eval_reference.npz — build container only (it runs the reference's own
detectron2/evaluation/pascal_voc_evaluation.py where it lies; nothing of it is copied).

    python tests/golden/make_voc_eval_golden.py

The reference module is loaded under stand-ins for detectron2.data (MetadataCatalog), detectron2.utils.comm,
detectron2.utils.file_io (PathManager) and the relative .evaluator import, with np.bool = bool (the module predates
NumPy 1.24).  Per case a small annotation tree is written into a temporary directory, the detections go through the
reference's own process() — so the text lines are the reference's — and voc_eval / voc_eval_corloc are called for both
AP forms and all ten thresholds.  Recorded per case: the inputs (detections in process() order, the objects in file
order) and rec / prec (per class and threshold, concatenated over the classes), ap07, ap12 and corloc as (10, C)
tables (corloc NaN where the reference raises ZeroDivisionError: detections of a class no image has a non-difficult
box of), and evaluate()'s dictionary where it does not raise.

Condition on the cases, asserted here: no two detections of a class share a quantised score (scores are drawn as
distinct thousandths), so the reference's result does not hang on its unstable argsort.  The cases hold difficult boxes,
a class without ground truth (with and without detections), a class without detections, an image whose only boxes of
a class are difficult, and two detections on one box."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
REF = "/root/reference/detectron2/evaluation/pascal_voc_evaluation.py"
OUT = os.path.join(HERE, "voc_eval_reference.npz")
NAMES = ["aeroplane", "bicycle", "bird", "boat", "bottle", "bus"]
META = {}


def reference_module():
    np.bool = bool
    mods = {n: types.ModuleType(n) for n in (
        "detectron2", "detectron2.data", "detectron2.utils", "detectron2.utils.comm", "detectron2.utils.file_io",
        "detectron2.evaluation", "detectron2.evaluation.evaluator")}
    mods["detectron2.evaluation"].__path__ = []
    mods["detectron2.data"].MetadataCatalog = types.SimpleNamespace(get=lambda name: META[name])
    mods["detectron2.utils"].comm = mods["detectron2.utils.comm"]
    mods["detectron2.utils.comm"].gather = lambda data, dst=0: [data]
    mods["detectron2.utils.comm"].is_main_process = lambda: True
    mods["detectron2.utils.file_io"].PathManager = types.SimpleNamespace(open=open, get_local_path=lambda p: p)
    mods["detectron2.evaluation.evaluator"].DatasetEvaluator = object
    sys.modules.update(mods)
    spec = importlib.util.spec_from_file_location("detectron2.evaluation.pascal_voc_evaluation", REF)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def make_case(seed):
    """-> (objects (M,7) rows (image, class, difficult, xmin, ymin, xmax, ymax) in file order, N, detections per image
    (boxes, scores, classes)).  Class 3 never has ground truth; class 4 never has detections; class 3 has detections
    in odd seeds only; image 0 holds only difficult boxes of class 0."""
    rng = np.random.default_rng(seed)
    C, N = len(NAMES), int(rng.integers(8, 14))
    objects = []
    for i in range(N):
        for _ in range(int(rng.integers(0, 6))):
            c = int(rng.choice([0, 1, 2, 4, 5]))
            x0, y0 = int(rng.integers(1, 300)), int(rng.integers(1, 200))
            w, h = int(rng.integers(20, 180)), int(rng.integers(20, 150))
            diff = int(rng.random() < 0.25)
            if i == 0 and c == 0:
                diff = 1
            objects.append([i, c, diff, x0, y0, x0 + w, y0 + h])
    objects.append([0, 0, 1, 40, 50, 140, 170])                    # image 0: class 0, difficult only
    objects.append([1, 1, 0, 30, 30, 130, 150])                    # two detections will sit on this one
    objects = np.asarray(objects, np.int64)
    per_class = {c: [] for c in range(C)}
    for c in range(C):
        if c == 4 or (c == 3 and seed % 2 == 0):
            continue
        n = int(rng.integers(150, 320))
        q = rng.choice(np.arange(1, 1000), n, replace=False)        # distinct thousandths
        score = (q / 1000.0 + rng.uniform(-3e-4, 3e-4, n)).astype(np.float32)
        of_c = objects[objects[:, 1] == c]
        for k in range(n):
            if len(of_c) and rng.random() < 0.6:                    # a jittered ground-truth box, 0-based xmin / ymin
                o = of_c[int(rng.integers(len(of_c)))]
                wh = np.array([o[5] - o[3], o[6] - o[4]], float)
                jit = rng.normal(0, 0.12, 4) * np.concatenate([wh, wh])
                box = np.array([o[3] - 1, o[4] - 1, o[5], o[6]], float) + jit
                im = int(o[0]) if rng.random() < 0.85 else int(rng.integers(N))
            else:
                x0, y0 = rng.uniform(0, 300), rng.uniform(0, 200)
                box = np.array([x0, y0, x0 + rng.uniform(10, 200), y0 + rng.uniform(10, 160)])
                im = int(rng.integers(N))
            per_class[c].append((im, box.astype(np.float32), score[k]))
    # two detections on one box
    per_class[1][0] = (1, np.array([29.2, 29.4, 130.3, 149.8], np.float32), per_class[1][0][2])
    per_class[1][1] = (1, np.array([28.7, 30.1, 129.6, 150.4], np.float32), per_class[1][1][2])
    dets = []
    for i in range(N):
        rows = [(b, s, c) for c in range(C) for (im, b, s) in per_class[c] if im == i]
        rows = [rows[j] for j in rng.permutation(len(rows))]
        dets.append((np.array([r[0] for r in rows], np.float32).reshape(-1, 4),
                     np.array([r[1] for r in rows], np.float32), np.array([r[2] for r in rows], np.int64)))
    return objects, N, dets


def write_tree(root, objects, N):
    ids = ["%06d" % (i + 1) for i in range(N)]
    os.makedirs(os.path.join(root, "VOC2007", "Annotations"))
    os.makedirs(os.path.join(root, "VOC2007", "ImageSets", "Main"))
    for year in ("2007", "2012"):
        os.makedirs(os.path.join(root, "results", "VOC" + year, "Main"))
    with open(os.path.join(root, "VOC2007", "ImageSets", "Main", "test.txt"), "w") as f:
        f.write("\n".join(ids) + "\n")
    for i, name in enumerate(ids):
        body = "".join(
            "<object><name>%s</name><pose>Unspecified</pose><truncated>0</truncated><difficult>%d</difficult>"
            "<bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>"
            % (NAMES[o[1]], o[2], o[3], o[4], o[5], o[6]) for o in objects if o[0] == i)
        with open(os.path.join(root, "VOC2007", "Annotations", name + ".xml"), "w") as f:
            f.write("<annotation><filename>%s.jpg</filename>%s</annotation>" % (name, body))
    return ids


def main():
    import voc_eval_ref as VR
    from jtsm_amd.structures import Boxes, Instances

    mod = reference_module()
    out = {}
    for case, seed in enumerate(range(1, 5)):
        objects, N, dets = make_case(seed)
        C = len(NAMES)
        boxes = np.concatenate([d[0] for d in dets])
        scores = np.concatenate([d[1] for d in dets])
        classes = np.concatenate([d[2] for d in dets]).astype(np.int32)
        images = np.concatenate([np.full(len(d[1]), i, np.int32) for i, d in enumerate(dets)])
        conf, _ = VR.through_text(boxes, scores)
        for c in range(C):
            v = conf[classes == c]
            assert len(np.unique(v)) == len(v), "equal quantised scores inside class %d" % c
        with tempfile.TemporaryDirectory() as root:
            ids = write_tree(root, objects, N)
            mod.parse_rec.cache_clear()
            for year in (2007, 2012):
                META["voc_%d_test" % year] = types.SimpleNamespace(
                    dirname=os.path.join(root, "VOC2007"), split="test", thing_classes=NAMES, year=year)
            ev = mod.PascalVOCDetectionEvaluator("voc_2007_test")
            ev.reset()
            inputs = [{"image_id": ids[i]} for i in range(N)]
            outputs = [{"instances": Instances((400, 500), pred_boxes=Boxes(torch.from_numpy(d[0])),
                                               scores=torch.from_numpy(d[1]), pred_classes=torch.from_numpy(d[2]))}
                       for d in dets]
            ev.process(inputs, outputs)
            anno = os.path.join(root, "VOC2007", "Annotations", "{}.xml")
            iset = os.path.join(root, "VOC2007", "ImageSets", "Main", "test.txt")
            tmpl = os.path.join(root, "{}.txt")
            rec, prec = [[] for _ in range(10)], [[] for _ in range(10)]
            ap07, ap12, corloc = np.zeros((10, C)), np.zeros((10, C)), np.zeros((10, C))
            with np.errstate(divide="ignore", invalid="ignore"):
                for c, name in enumerate(NAMES):
                    with open(tmpl.format(name), "w") as f:
                        f.write("\n".join(ev._predictions.get(c, [""])))
                    for t, thresh in enumerate(range(50, 100, 5)):
                        r, p, ap07[t, c] = mod.voc_eval(tmpl, anno, iset, name, ovthresh=thresh / 100.0, use_07_metric=True)
                        _, _, ap12[t, c] = mod.voc_eval(tmpl, anno, iset, name, ovthresh=thresh / 100.0, use_07_metric=False)
                        rec[t].append(r)
                        prec[t].append(p)
                        try:
                            corloc[t, c] = mod.voc_eval_corloc(tmpl, anno, iset, name, ovthresh=thresh / 100.0)
                        except ZeroDivisionError:
                            corloc[t, c] = np.nan
                name = "case%d" % case
                for year in (2007, 2012):
                    ev._dataset_name, ev._is_2007 = "voc_%d_test" % year, year == 2007
                    try:
                        res = ev.evaluate()
                        out["%s__result%d" % (name, year)] = np.array(
                            [res["bbox"][k] for k in ("AP", "AP50", "AP75")]
                            + [res["bbox CorLoc"][k] for k in ("CL", "CL50", "CL75")])
                    except ZeroDivisionError:
                        pass
        out[name + "__objects"], out[name + "__num_images"] = objects.astype(np.int32), np.int32(N)
        out[name + "__det_boxes"], out[name + "__det_scores"] = boxes, scores
        out[name + "__det_classes"], out[name + "__det_images"] = classes, images
        out[name + "__rec"] = np.stack([np.concatenate(r) for r in rec])
        out[name + "__prec"] = np.stack([np.concatenate(p) for p in prec])
        out[name + "__ap07"], out[name + "__ap12"], out[name + "__corloc"] = ap07, ap12, corloc
        print(name, "N=%d D=%d" % (N, len(scores)), "AP50(07) per class", np.round(ap07[0], 3),
              "recorded result:", [k for k in out if k.startswith(name + "__result")])
    np.savez_compressed(OUT, **out)
    print("-> %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
