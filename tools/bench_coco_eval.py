"""COCO box / mask AP on the device at a COCO val2017 shape: 5000 images, 80 categories, 100 detections and about 7
ground-truth objects per image, masks of 640 x 480.  All synthetic from a seed.  The predicted masks of a whole
dataset do not fit the device (5000 x 100 x 640 x 480 bytes), which is why the evaluator works per image; here a pool of
`--pool` images' boxes, masks and ground truth is rendered once on the device and image i uses entry i % pool with
scores of its own, so every image differs in its ranking and matching while the mask traffic per image is the real one.

Prints one JSON line and writes it to `--out`: device milliseconds per COCOEvaluator.process() image for the bbox task
and for bbox + segm (hipEvents around a pass over all images after `--warmup` images; a call is the Python wrapper, the
upload of the image's ground truth, the workspace allocation and every launch), milliseconds per evaluate() for both
tasks, the bytes of predicted masks an image has to read over the segm time as a share of the measured HBM copy rate,
the same two figures for the keypoints task alone at that shape (one `person` category, 17 keypoints with the COCO
sigmas, 20 kept detections and the same number of objects per image, each detected a few times with jitter),
and the host seconds of the NumPy restatement (tests/coco_eval_ref.py) on the first `--host-images` images with whether
the device's tables for those images agree bit for bit.  Needs the GPU; there is no fallback.

    python tools/bench_coco_eval.py [--images N] [--pool P] [--host-images N] [--warmup W] [--skip-host] [--out FILE]
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

H, W, N_IMAGES, K, N_DET = 480, 640, 5000, 80, 100
N_KEYPOINTS, N_DET_KP = 17, 20
HBM_COPY_BYTES_PER_S = 6.29e12          # the measured float4 copy rate of the MI355X (8.0 TB/s on paper)


def pool_entry(rng):
    """-> dict of NumPy arrays: gt_cats, gt_boxes (XYWH), gt_crowd, det_boxes (XYXY float32), det_classes for one pool
    image: about 7 objects, each detected a few times with jitter, the rest of the 100 detections at random."""
    G = int(rng.integers(3, 12))
    gb, gc = [], []
    for _ in range(G):
        side = float(rng.choice([rng.uniform(10, 30), rng.uniform(40, 90), rng.uniform(100, 300)]))
        w, h = min(side * rng.uniform(0.7, 1.3), W - 2), min(side * rng.uniform(0.7, 1.3), H - 2)
        gb.append([float(int(rng.uniform(0, W - w))), float(int(rng.uniform(0, H - h))), float(int(w)), float(int(h))])
        gc.append(int(rng.integers(K)) if rng.random() < 0.5 else int(rng.integers(5)))   # a few frequent categories
    boxes, classes = [], []
    for k in range(N_DET):
        if k < 4 * G:
            b, c = gb[k % G], gc[k % G]
            j = rng.normal(0, 0.08, 4) * np.array([b[2], b[3], b[2], b[3]])
            x, y, w, h = b[0] + j[0], b[1] + j[1], max(b[2] + j[2], 2), max(b[3] + j[3], 2)
        else:
            w, h = rng.uniform(8, 200), rng.uniform(8, 200)
            x, y, c = rng.uniform(0, W - w), rng.uniform(0, H - h), int(rng.integers(K))
        boxes.append([x, y, x + w, y + h])
        classes.append(c)
    return dict(gt_cats=np.array(gc, np.int64), gt_boxes=np.array(gb, np.float64),
                gt_crowd=(rng.random(G) < 0.05).astype(np.uint8), det_boxes=np.array(boxes, np.float32),
                det_classes=np.array(classes, np.int64))


def keypoint_pool_entry(rng):
    """-> dict of NumPy arrays for one pool image of the keypoints task: 3 to 11 persons (gt_boxes XYWH, gt_area,
    gt_crowd, gt_keypoints (G,17,3) with about a fifth of the points unlabelled and now and then a person without
    any), 20 detections (det_boxes XYXY float32, det_keypoints (20,17,3) float32): a person's points with jitter."""
    G = int(rng.integers(3, 12))
    gb, gk = [], []
    for _ in range(G):
        w, h = rng.uniform(30, 200), rng.uniform(60, 400)
        x, y = rng.uniform(0, W - w), rng.uniform(0, max(H - h, 1))
        xy = np.array([x, y]) + rng.random((N_KEYPOINTS, 2)) * np.array([w, h])
        v = rng.choice([0.0, 1.0, 2.0], N_KEYPOINTS, p=[0.2, 0.2, 0.6]) * (rng.random() > 0.1)
        gb.append([x, y, w, h])
        gk.append(np.concatenate([np.round(xy), v[:, None]], 1))
    gb, gk = np.array(gb, np.float64), np.array(gk, np.float64)
    boxes, kps = [], []
    for k in range(N_DET_KP):
        b, kp = gb[k % G], gk[k % G]
        j = rng.normal(0, 0.03, (N_KEYPOINTS, 2)) * b[2:]
        boxes.append([b[0], b[1], b[0] + b[2], b[1] + b[3]])
        kps.append(np.concatenate([kp[:, :2] + 0.5 + j, rng.random((N_KEYPOINTS, 1))], 1))
    return dict(gt_cats=np.zeros(G, np.int64), gt_boxes=gb, gt_area=gb[:, 2] * gb[:, 3] * 0.5,
                gt_crowd=(rng.random(G) < 0.05).astype(np.uint8), gt_keypoints=gk,
                det_boxes=np.array(boxes, np.float32), det_keypoints=np.array(kps, np.float32))


def rasterise(boxes_xyxy, dev):
    """(n,4) boxes -> (n,H,W) bool rectangles on the device (rounded to pixel edges)."""
    b = torch.as_tensor(np.asarray(boxes_xyxy, np.float32)).to(dev).round()
    xx = torch.arange(W, device=dev).view(1, 1, W)
    yy = torch.arange(H, device=dev).view(1, H, 1)
    x0, y0, x1, y1 = (b[:, k].view(-1, 1, 1) for k in range(4))
    return (xx >= x0) & (xx < x1) & (yy >= y0) & (yy < y1)


def keypoints_run(a, dev, rng, ids):
    """The keypoints task alone, timed as the other two -> (ms per process() image, ms per evaluate(), results)."""
    from jtsm_amd.evaluation import COCOEvaluator, COCOGroundTruth
    from jtsm_amd.structures import Boxes, Instances

    pool = [keypoint_pool_entry(rng) for _ in range(a.pool)]
    for p in pool:
        p["dev_boxes"] = torch.from_numpy(p["det_boxes"]).to(dev)
        p["dev_keypoints"] = torch.from_numpy(p["det_keypoints"]).to(dev)
        p["dev_classes"] = torch.zeros(N_DET_KP, dtype=torch.int64, device=dev)
    scores = torch.from_numpy((rng.integers(1, 1000, (a.images, N_DET_KP)) / 1000.0).astype(np.float32)).to(dev)
    gt = COCOGroundTruth(1)
    for i in range(a.images):
        p = pool[i % a.pool]
        gt.add(ids[i], p["gt_cats"], p["gt_boxes"], p["gt_area"], p["gt_crowd"], keypoints=p["gt_keypoints"])

    def one(ev, i):
        p = pool[i % a.pool]
        ev.process([{"image_id": ids[i]}], [{"instances": Instances(
            (H, W), pred_boxes=Boxes(p["dev_boxes"]), scores=scores[i], pred_classes=p["dev_classes"],
            pred_keypoints=p["dev_keypoints"])}])

    for i in range(min(a.warmup, a.images)):                           # warm-up on a throw-away evaluator
        one(COCOEvaluator(gt, tasks=("keypoints",), device=dev), i)
    ev = COCOEvaluator(gt, tasks=("keypoints",), device=dev)
    torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    for i in range(a.images):
        one(ev, i)
    e[1].record()
    res = ev.evaluate()
    e[2].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]) / max(a.images, 1), e[1].elapsed_time(e[2]), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=N_IMAGES)
    ap.add_argument("--pool", type=int, default=8)
    ap.add_argument("--host-images", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coco_eval_bench.json"))
    a = ap.parse_args()
    import coco_eval_ref as CR
    from jtsm_amd.evaluation import COCOEvaluator, COCOGroundTruth
    from jtsm_amd.structures import Boxes, Instances

    assert torch.cuda.is_available(), "bench_coco_eval needs the MI355X"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    pool = [pool_entry(rng) for _ in range(a.pool)]
    for p in pool:
        gxyxy = p["gt_boxes"].copy()
        gxyxy[:, 2:] += gxyxy[:, :2]
        p["gt_masks"] = rasterise(gxyxy, dev).cpu().numpy()
        p["gt_area"] = p["gt_masks"].reshape(len(gxyxy), -1).sum(1).astype(np.float64)
        p["dev_boxes"] = torch.from_numpy(p["det_boxes"]).to(dev)
        p["dev_classes"] = torch.from_numpy(p["det_classes"]).to(dev)
        p["dev_masks"] = rasterise(p["det_boxes"], dev)
    scores = (rng.integers(1, 1000, (a.images, N_DET)) / 1000.0).astype(np.float32)
    dev_scores = torch.from_numpy(scores).to(dev)
    ids = list(range(a.images))

    def ground_truth(n_images, masks):
        gt = COCOGroundTruth(K)
        for i in range(n_images):
            p = pool[i % a.pool]
            gt.add(ids[i], p["gt_cats"], p["gt_boxes"], p["gt_area"], p["gt_crowd"], p["gt_masks"] if masks else None)
        return gt

    def instances(i, masks):
        p = pool[i % a.pool]
        inst = Instances((H, W), pred_boxes=Boxes(p["dev_boxes"]), scores=dev_scores[i], pred_classes=p["dev_classes"])
        if masks:
            inst.set("pred_masks", p["dev_masks"])
        return inst

    def run(n_images, masks, gt):
        """-> (ms per process() image, ms per evaluate(), evaluator, results)"""
        ev = COCOEvaluator(gt, device=dev)
        for i in range(min(a.warmup, n_images)):                       # warm-up on a throw-away evaluator
            COCOEvaluator(gt, device=dev).process([{"image_id": ids[i]}], [{"instances": instances(i, masks)}])
        torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        for i in range(n_images):
            ev.process([{"image_id": ids[i]}], [{"instances": instances(i, masks)}])
        e[1].record()
        res = ev.evaluate()
        e[2].record()
        torch.cuda.synchronize()
        return e[0].elapsed_time(e[1]) / max(n_images, 1), e[1].elapsed_time(e[2]), ev, res

    gt_masks = ground_truth(a.images, True)
    bbox_ms, bbox_eval_ms, _, res_b = run(a.images, False, gt_masks)
    both_ms, both_eval_ms, _, res_s = run(a.images, True, gt_masks)
    kp_ms, kp_eval_ms, res_k = keypoints_run(a, dev, rng, ids)
    mask_bytes = N_DET * H * W
    segm_ms = max(both_ms - bbox_ms, 1e-9)
    line = {"workload": "COCO val2017 shape: %d images of %d x %d, %d categories, %d detections and %.1f ground-truth "
                        "objects per image (a pool of %d rendered images, scores per image)"
                        % (a.images, W, H, K, N_DET, np.mean([len(pool[i % a.pool]["gt_cats"]) for i in range(a.images)]),
                           a.pool),
            "process_image_bbox_ms": round(bbox_ms, 4), "process_image_bbox_and_segm_ms": round(both_ms, 4),
            "evaluate_bbox_ms": round(bbox_eval_ms, 3), "evaluate_bbox_and_segm_ms": round(both_eval_ms, 3),
            "pred_mask_bytes_per_image": mask_bytes,
            "segm_share_of_hbm_copy_rate": round(mask_bytes / (segm_ms * 1e-3) / HBM_COPY_BYTES_PER_S, 4),
            "hbm_copy_rate_bytes_per_s": HBM_COPY_BYTES_PER_S,
            "keypoints_workload": "one category, %d keypoints (COCO sigmas), %d detections per image"
                                  % (N_KEYPOINTS, N_DET_KP),
            "process_image_keypoints_ms": round(kp_ms, 4), "evaluate_keypoints_ms": round(kp_eval_ms, 3),
            "keypoints": {k: round(v, 4) for k, v in res_k["keypoints"].items()},
            "bbox": {k: round(v, 4) for k, v in res_b["bbox"].items()},
            "segm": {k: round(v, 4) for k, v in res_s["segm"].items()}}
    if not a.skip_host:
        n = min(a.host_images, a.images)
        _, _, ev, _ = run(n, True, ground_truth(n, True))
        dataset = []
        for i in range(n):
            p = pool[i % a.pool]
            if "host_masks" not in p:
                p["host_masks"] = p["dev_masks"].cpu().numpy()
            dataset.append(dict(image_id=ids[i], det_boxes=p["det_boxes"], det_scores=scores[i],
                                det_classes=p["det_classes"], det_masks=p["host_masks"],
                                gt_cats=p["gt_cats"], gt_boxes=p["gt_boxes"], gt_area=p["gt_area"],
                                gt_crowd=p["gt_crowd"], gt_masks=p["gt_masks"]))
        t0 = time.perf_counter()
        _, tables = CR.evaluate(dataset, K, ("bbox", "segm"))
        line["restatement_host_images"] = n
        line["restatement_host_s"] = round(time.perf_counter() - t0, 2)
        bits = lambda x: np.ascontiguousarray(x).view(np.int64)  # noqa: E731
        line["tables_equal"] = bool(all(np.array_equal(bits(ev.last_eval[t][k]), bits(tables[t][k]))
                                        for t in ("bbox", "segm") for k in ("precision", "scores", "recall")))
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
