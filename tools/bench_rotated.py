"""The two rotated-box operators alone.  Prints one JSON line: ms per `pairwise_iou_rotated` call at 2000 x 2000
clustered boxes and ms per `batched_nms_rotated` call at the RRPN shape (3 levels x 2000 boxes, threshold 0.7) —
wrapper, allocations and every launch included; events around `--calls` calls after 3 — and, beside them, the NumPy
restatement's time (tests/rotated_ref.py) on this box's host for the same inputs, with the agreement of the results.
--out writes the same JSON to a file.

    python tools/bench_rotated.py [--calls C] [--out profiles/rotated_bench.json]
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


def timed(fn, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import rotated_ref as R
    from jtsm_amd.layers import batched_nms_rotated, pairwise_iou_rotated

    dev = torch.device("cuda", 0)
    both = R.clustered_boxes(4000, 1, with_scores=False)[0]
    b1, b2 = both[:2000], both[2000:]
    t1, t2 = torch.from_numpy(b1).to(dev), torch.from_numpy(b2).to(dev)
    iou_ms = timed(lambda: pairwise_iou_rotated(t1, t2), a.calls)
    got = pairwise_iou_rotated(t1, t2).cpu().numpy()
    t0 = time.perf_counter()
    want = R.iou_matrix(b1, b2)
    ref_iou_ms = (time.perf_counter() - t0) * 1e3

    boxes = R.clustered_boxes(6000, 2, with_scores=False)[0]
    scores = ((np.random.RandomState(3).permutation(6000) + 0.5) / 6000.0).astype(np.float32)     # no ties
    levels = np.repeat(np.arange(3, dtype=np.int64), 2000)
    tb, ts, tl = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), torch.from_numpy(levels).to(dev)
    nms_ms = timed(lambda: batched_nms_rotated(tb, ts, tl, 0.7), a.calls)
    keep = batched_nms_rotated(tb, ts, tl, 0.7).cpu().numpy()
    t0 = time.perf_counter()
    ref_keep = R.batched_nms(boxes, scores, levels, 0.7)
    ref_nms_ms = (time.perf_counter() - t0) * 1e3

    out = {"workload": "rotated boxes piled on 6 rectangles: IoU 2000 x 2000; NMS 3 levels x 2000 boxes at 0.7",
           "pairwise_iou_rotated_ms_per_call": round(iou_ms, 4), "batched_nms_rotated_ms_per_call": round(nms_ms, 4),
           "numpy_iou_ms": round(ref_iou_ms, 1), "numpy_nms_ms": round(ref_nms_ms, 1),
           "iou_max_abs_diff": float(np.abs(got.astype(np.float64) - want).max()),
           "iou_bit_equal_share": float(np.mean(got == want)), "iou_nonzero_pairs": int((want > 0).sum()),
           "nms_kept": int(keep.size), "nms_keep_identical": bool(np.array_equal(keep, ref_keep)), "calls": a.calls}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
