"""Pascal VOC evaluation on the device at VOC07-test shape: 4952 images, 20 classes, 100 detections per image
(495 200 detections spread over the classes, scores with three significant decimals' worth of ties), a few boxes per
image as ground truth, all synthetic from a seed.  Prints one JSON line: device milliseconds per
PascalVOCDetectionEvaluator.evaluate() (concatenation, the jtsm_voc_eval call, the one read-back; hipEvents around
`--steps` calls after `--warmup`), the same for the library call alone, and the host seconds of the NumPy restatement
of the reference (tests/voc_eval_ref.py: one run, text formatting included) on the same input, with whether the two
agree (11-point AP and CorLoc tables bit for bit).  Needs the GPU; there is no fallback.

    python tools/bench_voc_eval.py [--steps N] [--warmup W] [--year 2007|2012] [--skip-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_IMAGES, N_CLASSES, PER_IMAGE = 4952, 20, 100


def synthetic(seed=0):
    rng = np.random.default_rng(seed)
    objects = []
    for i in range(N_IMAGES):
        for _ in range(int(rng.integers(1, 6))):
            x0, y0 = int(rng.integers(1, 350)), int(rng.integers(1, 250))
            objects.append([i, int(rng.integers(N_CLASSES)), int(rng.random() < 0.15), x0, y0,
                            x0 + int(rng.integers(20, 150)), y0 + int(rng.integers(20, 120))])
    objects = np.asarray(objects, np.int64)
    by_image = np.split(objects, np.cumsum(np.bincount(objects[:, 0], minlength=N_IMAGES))[:-1])
    D = N_IMAGES * PER_IMAGE
    images = np.repeat(np.arange(N_IMAGES, dtype=np.int32), PER_IMAGE)
    boxes = np.empty((D, 4), np.float32)
    classes = rng.integers(0, N_CLASSES, D).astype(np.int32)
    scores = (rng.random(D) ** 3).astype(np.float32)
    x0, y0 = rng.uniform(0, 350, D), rng.uniform(0, 250, D)
    boxes[:] = np.stack([x0, y0, x0 + rng.uniform(10, 150, D), y0 + rng.uniform(10, 120, D)], 1)
    near = rng.random(D) < 0.3                      # some detections sit on an object of their image
    for d in np.nonzero(near)[0]:
        o = by_image[images[d]]
        o = o[int(rng.integers(len(o)))]
        boxes[d] = np.array([o[3] - 1, o[4] - 1, o[5], o[6]], float) + rng.normal(0, 4, 4)
        classes[d] = o[1]
    return objects, boxes, scores, classes, images


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--year", type=int, default=2007)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    import voc_eval_ref as VR
    from jtsm_amd.evaluation import PascalVOCDetectionEvaluator, VOCGroundTruth
    from jtsm_amd.evaluation import pascal_voc_evaluation as PV
    from jtsm_amd.structures import Boxes, Instances

    assert torch.cuda.is_available(), "bench_voc_eval needs the MI355X"
    dev = torch.device("cuda:0")
    objects, boxes, scores, classes, images = synthetic()
    ids = ["%06d" % i for i in range(N_IMAGES)]
    gt = VOCGroundTruth(ids, objects, N_CLASSES)
    ev = PascalVOCDetectionEvaluator(["c%02d" % c for c in range(N_CLASSES)], gt, a.year, device=dev)
    tb, ts, tc = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), torch.from_numpy(classes).to(dev)
    batch = 8                                       # process() as a loader would call it
    for lo in range(0, N_IMAGES, batch):
        hi = min(lo + batch, N_IMAGES)
        ev.process([{"image_id": ids[i]} for i in range(lo, hi)],
                   [{"instances": Instances((375, 500), pred_boxes=Boxes(tb[i * PER_IMAGE:(i + 1) * PER_IMAGE]),
                                            scores=ts[i * PER_IMAGE:(i + 1) * PER_IMAGE],
                                            pred_classes=tc[i * PER_IMAGE:(i + 1) * PER_IMAGE])} for i in range(lo, hi)])

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps, out

    ms_eval, result = timed(ev.evaluate)
    ti = torch.from_numpy(images).to(dev)
    ms_call, out = timed(lambda: PV.voc_eval(tb, ts, tc, ti, ev._gt_dev, N_IMAGES, N_CLASSES, a.year == 2007))
    line = {"workload": "VOC07-test shape: %d images, %d classes, %d detections per image, %d ground-truth boxes"
                        % (N_IMAGES, N_CLASSES, PER_IMAGE, len(objects)),
            "year": a.year, "evaluate_ms": round(ms_eval, 3), "voc_eval_call_ms": round(ms_call, 3),
            "result": {g: {k: round(float(v), 4) for k, v in d.items()} for g, d in result.items()}}
    if not a.skip_host:
        t0 = time.perf_counter()
        want = VR.evaluate(boxes, scores, classes, images, gt.gt_boxes, gt.gt_difficult, gt.gt_offsets, N_IMAGES,
                           N_CLASSES, a.year == 2007)
        line["restatement_host_s"] = round(time.perf_counter() - t0, 2)
        got_ap, got_cl, _, got_counts = PV.split_tables(out["tables"].cpu(), N_CLASSES)
        line["corloc_and_counts_equal"] = bool(np.array_equal(got_cl, want["corloc"]) and np.array_equal(got_counts, want["counts"]))
        if a.year == 2007:
            line["ap_equal"] = bool(np.array_equal(got_ap, want["ap"]))
        else:
            line["ap_max_abs_diff"] = float(np.abs(got_ap - want["ap"]).max())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
