"""One C-MIL training step of the shipped configuration (tests/golden/configs/cmil_WSR_18_DC5_1x.yaml): B=2 synthetic
3x1024x1024 images, 2000 clustered proposals each, 20 classes, ROILoopPool, three refinement branches.  Prints one JSON
line: ms/step and img/s (events around `--steps` steps after `--warmup`), then — on the last step's own inputs — ms per
`roi_merge` call and per `roi_label` call (wrapper, allocations and every launch included; events around `--calls`
calls after 3), and the NumPy restatement's time (tests/cmil_ref.py) on this box's host for the same inputs, with the
agreement of their integer results.  --out writes the same JSON to a file.

    python tools/bench_cmil.py [--steps N] [--warmup W] [--calls C] [--iter I] [--out profiles/cmil_bench.json]
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--iter", type=int, default=2500, help="ROIMerge.cur_iter of the timed steps (lambda 0.64)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import cmil_ref as CR
    from jtsm_amd.config import add_wsl_config, get_cfg
    from jtsm_amd.layers.cmil import roi_label, roi_merge
    from jtsm_amd.modeling import build_model
    from jtsm_amd.modeling.roi_heads.roi_heads import bag_offsets
    from jtsm_amd.modeling.roi_heads.roi_heads_jtsm import class_lists
    from model_util import to_batched_inputs
    from oracle import model as OM

    B, R = 2, 2000
    cfg = get_cfg()
    add_wsl_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "tests", "golden", "configs", "cmil_WSR_18_DC5_1x.yaml"))
    cfg.MODEL.DEVICE = "cuda"
    model = build_model(cfg)
    with torch.no_grad():
        model.backbone.stem.conv1.weight.mul_(1.0 / 64)
    model.train()
    merge = model.roi_heads.box_predictor.roi_merge
    batch = OM.synthetic_batch(1234, B=B, size=1024, R=R, sp_block=32, n_stuff=1, nt=20, ns=2, cluster=1.0, objects=40)
    inputs = to_batched_inputs(batch)
    for x in inputs:
        x["image"] = x["image"].to(torch.uint8).cuda()
        x["proposals"] = x["proposals"].to("cuda")
        x["instances"] = x["instances"].to("cuda")
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=1e-7, momentum=0.9)

    def step():
        merge.cur_iter = a.iter
        opt.zero_grad(set_to_none=True)
        losses = model(inputs)
        sum(losses.values()).backward()
        opt.step()
        return losses

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        losses = step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps

    # ---- the two operators alone, on the step's own inputs
    heads = model.roi_heads
    aux = heads.aux
    counts = [R] * B
    dev = aux["mil_scores"].device
    offsets = bag_offsets(counts, dev)
    boxes = torch.cat([x["proposals"].proposal_boxes.tensor for x in inputs]).contiguous()
    S, scores, probs, lam = aux["merge_scores"], aux["mil_scores"], aux["img_probs"], aux["merge_lambda"]
    g = torch.Generator(device=dev).manual_seed(7)
    C, D = torch.randn(B * R, 20, device=dev, generator=g), torch.randn(B * R, 20, device=dev, generator=g)
    cls, cnt = class_lists(heads.gt_classes_img_oh)
    perm = aux["perm_r0"]
    merge_ms = timed(lambda: roi_merge(S, boxes, C, D, offsets, lam, R), a.calls)
    label_ms = timed(lambda: roi_label(scores, boxes, offsets, cls, cnt, probs, perm=perm, num_classes=20), a.calls)
    _, _, I, IC, moff = roi_merge(S, boxes, C, D, offsets, lam, R)
    lab = roi_label(scores, boxes, offsets, cls, cnt, probs, perm=perm, num_classes=20)

    # ---- the NumPy restatement on this box's host, same inputs
    h = lambda t: t.cpu().numpy()  # noqa: E731
    hS, hb, hC, hD, hoff = h(S), h(boxes), h(C), h(D), h(offsets)
    t0 = time.perf_counter()
    want = CR.roi_merge(hS, hb, hC, hD, hoff, np.float32(lam))
    ref_merge_ms = (time.perf_counter() - t0) * 1e3
    hsc, hp, hperm, hcls, hcnt = h(scores), h(probs), h(perm), h(cls), h(cnt)
    t0 = time.perf_counter()
    ref_lab = [CR.roi_label_image(hsc[hoff[b]:hoff[b + 1]], hb[hoff[b]:hoff[b + 1]], hcls[b, :hcnt[b]], hp[b],
                                  hperm[hoff[b]:hoff[b + 1]], num_classes=20) for b in range(B)]
    ref_label_ms = (time.perf_counter() - t0) * 1e3
    live = int(want["merged_offsets"][-1])
    out = {"workload": "C-MIL WSR-18 DC5, %d x 3x1024x1024, %d proposals each, 20 classes, ROILoopPool, 3 branches" % (B, R),
           "ms_per_step": round(ms, 3), "img_per_s": round(1000.0 * B / ms, 2),
           "roi_merge_ms_per_call": round(merge_ms, 4), "roi_label_ms_per_call": round(label_ms, 4),
           "numpy_roi_merge_ms": round(ref_merge_ms, 2), "numpy_roi_label_ms": round(ref_label_ms, 2),
           "lambda": lam, "merged_rows": live, "largest_clique": int(want["IC"].max()),
           "merge_integers_identical": bool(np.array_equal(h(I), want["I"]) and np.array_equal(h(IC), want["IC"])
                                            and np.array_equal(h(moff), want["merged_offsets"])),
           "labels_identical": bool(np.array_equal(h(lab["labels"]), np.concatenate([r["labels"] for r in ref_lab]))),
           "host_round_trips_per_step": 0,
           "losses": {k: round(float(v.detach()), 6) for k, v in losses.items()}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
