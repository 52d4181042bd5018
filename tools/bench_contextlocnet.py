"""One ContextLocNet training step of the shipped configuration (tests/golden/configs/contextlocnet_WSR_18_DC5_1x.yaml):
B=2 synthetic 3x1024x1024 images, 2000 clustered proposals each, 20 classes (12 000 pooled rows); --reference-shape:
1 image, 4000 proposals.  Prints one JSON line: ms/step, img/s, the ROILoopPool forward's time (hipEvents) and output
bytes, and the box head's time (DAN + cls / det forward).

    python tools/bench_contextlocnet.py [--steps N] [--warmup W] [--reference-shape]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reference-shape", action="store_true")
    a = ap.parse_args()
    from jtsm_amd import _lib as L
    from jtsm_amd.config import add_wsl_config, get_cfg
    from jtsm_amd.modeling import build_model
    from model_util import to_batched_inputs
    from oracle import model as OM

    B, R = (1, 4000) if a.reference_shape else (2, 2000)
    cfg = get_cfg()
    add_wsl_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "tests", "golden", "configs", "contextlocnet_WSR_18_DC5_1x.yaml"))
    cfg.MODEL.DEVICE = "cuda"
    model = build_model(cfg)
    with torch.no_grad():
        model.backbone.stem.conv1.weight.mul_(1.0 / 64)
    model.train()
    batch = OM.synthetic_batch(1234, B=B, size=1024, R=R, sp_block=32, n_stuff=1, nt=20, ns=2, cluster=1.0, objects=40)
    inputs = to_batched_inputs(batch)
    for x in inputs:
        x["image"] = x["image"].to(torch.uint8).cuda()
        x["proposals"] = x["proposals"].to("cuda")
        x["instances"] = x["instances"].to("cuda")
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=1e-7, momentum=0.9)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = sum(model(inputs).values())
        loss.backward()
        opt.step()
        return loss

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        loss = step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    # one more step with the library's per-call hipEvents: the pool's forward, and the box head (DAN + predictors)
    head = model.roi_heads.box_head
    spans = []
    orig = head.forward

    def timed_head(*args, **kw):
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0.record()
        out = orig(*args, **kw)
        s1.record()
        spans.append((s0, s1))
        return out

    head.forward = timed_head
    L.TIMING = []
    try:
        step()
        torch.cuda.synchronize()
        pool = [(span.ms(), nb) for n, span, nb in L.TIMING if n == "jtsm_roi_loop_pool_forward_f32"]
    finally:
        L.TIMING = None
        head.forward = orig
    out_bytes = 3 * B * R * 512 * 49 * 4
    print(json.dumps({"workload": "ContextLocNet WSR-18 DC5, %d x 3x1024x1024, %d proposals each, 20 classes" % (B, R),
                      "ms_per_step": round(ms, 3), "img_per_s": round(1000.0 * B / ms, 2),
                      "roi_loop_pool_fwd_ms": round(sum(t for t, _ in pool), 4), "roi_loop_pool_out_bytes": out_bytes,
                      "box_head_fwd_ms": round(sum(s0.elapsed_time(s1) for s0, s1 in spans), 4),
                      "pooled_rows": 3 * B * R, "final_loss": round(float(loss), 6)}))


if __name__ == "__main__":
    main()
