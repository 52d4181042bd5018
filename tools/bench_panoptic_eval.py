"""Panoptic-quality and semantic confusion accumulation on the device at a COCO-panoptic shape: 500 images of
640 x 480, 133 categories (80 things, 53 stuff), about 20 ground-truth and about 20 predicted segments per image (a
jittered 4 x 5 grid, the prediction shifted so that matches fall on both sides of IoU 0.5), 53 semantic classes; all
synthetic from a seed and uploaded before the clock starts.  Prints one JSON line and writes it to `--out`: device
milliseconds per jtsm_pq_accumulate call and per jtsm_confusion_accumulate call (hipEvents around `--steps` passes over
the images after `--warmup`; each call is the Python wrapper, its workspace allocation and every launch of the entry
point), the bytes of the two maps each call has to read over that time as a share of the measured HBM copy rate, and
the host seconds of the NumPy restatement (tests/pq_ref.py: np.unique / np.bincount per image) on the same input with
whether the totals agree bit for bit.  Needs the GPU; there is no fallback.

    python tools/bench_panoptic_eval.py [--steps N] [--warmup W] [--images N] [--skip-host] [--out FILE]
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

H, W, N_IMAGES = 480, 640, 500
N_THINGS, N_STUFF = 80, 53
N_CAT = N_THINGS + N_STUFF
HBM_COPY_BYTES_PER_S = 6.29e12          # the measured float4 copy rate of the MI355X (8.0 TB/s on paper)


def synthetic_image(rng):
    """-> pred (H,W) int32, pred_table (P,5), gt (H,W) int32, gt_table (G,2), sem_pred (H,W) int64, sem_gt (H,W) uint8."""
    ys = np.sort(np.concatenate([[0, H], rng.integers(H // 8, H - H // 8, 3)]))
    xs = np.sort(np.concatenate([[0, W], rng.integers(W // 8, W - W // 8, 4)]))
    gt, pred = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    gt_table, pred_table = [], []
    for r in range(4):
        for c in range(5):
            y0, y1, x0, x1 = ys[r], ys[r + 1], xs[c], xs[c + 1]
            if y1 - y0 < 2 or x1 - x0 < 2 or rng.random() < 0.05:
                continue
            cat = int(rng.integers(N_CAT))
            gt_table.append([cat, int(rng.random() < 0.05)])
            gt[y0:y1, x0:x1] = len(gt_table)
            dy, dx = (int(round(rng.uniform(-0.3, 0.3) * s)) for s in (y1 - y0, x1 - x0))
            region = pred[max(y0 + dy, 0):max(y1 + dy, 0), max(x0 + dx, 0):max(x1 + dx, 0)]
            if region.size == 0:
                continue
            pcat = cat if rng.random() < 0.9 else int(rng.integers(N_CAT))
            sid = 1 + len(pred_table)
            region[...] = sid
            isthing = pcat < N_THINGS
            pred_table.append([sid, int(isthing), pcat if isthing else pcat - N_THINGS, sid - 1 if isthing else -1, 0])
    pred_table = [row for row in pred_table if (pred == row[0]).any()]
    sem_gt = (gt % N_STUFF).astype(np.uint8)
    sem_gt[gt == 0] = 255
    sem_pred = (pred % N_STUFF).astype(np.int64)
    return (pred, np.array(pred_table, np.int32).reshape(-1, 5), gt, np.array(gt_table, np.int32).reshape(-1, 2), sem_pred,
            sem_gt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--images", type=int, default=N_IMAGES)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panoptic_eval_bench.json"))
    a = ap.parse_args()
    import pq_ref as PR
    from jtsm_amd.evaluation import panoptic_evaluation as PE
    from jtsm_amd.evaluation import sem_seg_evaluation as SE

    assert torch.cuda.is_available(), "bench_panoptic_eval needs the MI355X"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    host = [synthetic_image(rng) for _ in range(a.images)]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    images = [tuple(up(x) for x in im) + (torch.full((1,), len(im[1]), dtype=torch.int32, device=dev),) for im in host]
    thing_cat, stuff_cat = list(range(N_THINGS)), [N_THINGS + k for k in range(N_STUFF)]
    tc, sc = up(np.array(thing_cat, np.int32)), up(np.array(stuff_cat, np.int32))

    def pq_pass():
        totals = PE.new_totals(N_CAT, dev)
        for pred, table, gt, gt_table, _, _, n in images:
            PE.pq_accumulate(pred, table, n, tc, sc, gt, gt_table, totals)
        return totals

    def conf_pass():
        conf = torch.zeros((N_STUFF + 1) ** 2 + 1, dtype=torch.int64, device=dev)
        for _, _, _, _, sem_pred, sem_gt, _ in images:
            SE.confusion_accumulate(sem_pred, sem_gt, N_STUFF, 255, conf)
        return conf

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
        return e0.elapsed_time(e1) / (a.steps * len(images)), out

    pq_ms, totals = timed(pq_pass)
    conf_ms, conf = timed(conf_pass)
    pq_bytes, conf_bytes = H * W * (4 + 4), H * W * (8 + 1)
    share = lambda nbytes, ms: nbytes / (ms * 1e-3) / HBM_COPY_BYTES_PER_S  # noqa: E731
    line = {"workload": "COCO-panoptic shape: %d images of %d x %d, %d categories, %.1f ground-truth and %.1f predicted "
                        "segments per image, %d semantic classes"
                        % (len(images), W, H, N_CAT, np.mean([len(im[3]) for im in host]),
                           np.mean([len(im[1]) for im in host]), N_STUFF),
            "pq_accumulate_call_ms": round(pq_ms, 4), "confusion_accumulate_call_ms": round(conf_ms, 4),
            "pq_map_bytes_per_call": pq_bytes, "confusion_map_bytes_per_call": conf_bytes,
            "pq_call_share_of_hbm_copy_rate": round(share(pq_bytes, pq_ms), 4),
            "confusion_call_share_of_hbm_copy_rate": round(share(conf_bytes, conf_ms), 4),
            "hbm_copy_rate_bytes_per_s": HBM_COPY_BYTES_PER_S}
    tp, fp, fn, iou_sum, stats = PE.split_totals(totals["tables"].cpu(), N_CAT)
    line["totals"] = {"tp": int(tp.sum()), "fp": int(fp.sum()), "fn": int(fn.sum()), "stats": stats.tolist()}
    if not a.skip_host:
        t0 = time.perf_counter()
        want = PR.pq_accumulate([(im[0], im[1], len(im[1]), im[2], im[3]) for im in host], thing_cat, stuff_cat, N_CAT)
        line["pq_restatement_host_s"] = round(time.perf_counter() - t0, 2)
        t0 = time.perf_counter()
        want_conf = sum(PR.confusion(im[4], im[5], N_STUFF, 255) for im in host)
        line["confusion_restatement_host_s"] = round(time.perf_counter() - t0, 2)
        line["pq_totals_equal"] = bool(all(np.array_equal(g, want[k]) for g, k in ((tp, "tp"), (fp, "fp"), (fn, "fn"), (stats, "stats")))
                                       and np.array_equal(iou_sum.view(np.int64), want["iou_sum"].view(np.int64)))
        got_conf = conf.cpu().numpy()
        line["confusion_equal"] = bool(got_conf[-1] == 0 and np.array_equal(got_conf[:-1].reshape(N_STUFF + 1, -1), want_conf))
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
