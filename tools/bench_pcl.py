"""One PCL training step of the shipped configuration (tests/golden/configs/pcl_WSR_18_DC5_1x.yaml): B=2 synthetic
3x1024x1024 images, 2000 clustered proposals each, 20 classes, three refinement branches; --reference-shape: 1 image,
4000 proposals (the reference clusters one image per process).  Prints one JSON line: ms/step, img/s, and from one
more step under the library's per-call hipEvents the time inside the ROIPool forward, the clustering launches
(jtsm_pcl_cluster_f32: centre search, assignment, cluster statistics) and the loss launches (soft-max, loss forward,
loss backward), summed over the three branches.

    python tools/bench_pcl.py [--steps N] [--warmup W] [--reference-shape]
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
    cfg.merge_from_file(os.path.join(ROOT, "tests", "golden", "configs", "pcl_WSR_18_DC5_1x.yaml"))
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
    L.TIMING = []
    try:
        step()
        torch.cuda.synchronize()
        spans = [(n, span.ms()) for n, span, _ in L.TIMING]
    finally:
        L.TIMING = None
    total = lambda *names: round(sum(t for n, t in spans if n in names), 4)  # noqa: E731
    tables = model.roi_heads.aux["pcl_tables"]
    print(json.dumps({"workload": "PCL WSR-18 DC5, %d x 3x1024x1024, %d proposals each, 20 classes, 3 branches" % (B, R),
                      "ms_per_step": round(ms, 3), "img_per_s": round(1000.0 * B / ms, 2),
                      "roi_pool_fwd_ms": total("jtsm_roi_pool_forward_f32"),
                      "pcl_cluster_ms": total("jtsm_pcl_cluster_f32"),
                      "pcl_loss_ms": total("jtsm_pcl_softmax_f32", "jtsm_pcl_loss_forward_f32", "jtsm_pcl_loss_backward_f32"),
                      "clusters_per_branch": [int(t["pc_num"].sum()) for t in tables],
                      "losses": {k: round(float(v), 6) for k, v in losses.items()}}))


if __name__ == "__main__":
    main()
