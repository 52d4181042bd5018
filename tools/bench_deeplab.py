"""DeepLab v3+ at the benchmark size.  Prints one JSON line: ms per full training step (forward, backward and SGD) and
images / s of deeplab_v3_plus_R_103_os16_mg124_poly_90k_bs16 (the flattened shipped configuration under
tests/golden/configs/) on 2 x 3 x 512 x 1024 synthetic crops; and, per call with wrapper, allocations and every launch
included (events around `--calls` calls after 3),
  * batch norm + ReLU forward + backward at (2, 256, 128, 256),
  * the hard-pixel loss forward + backward at N = 2, C = 19, 128 x 256 -> 512 x 1024,
each beside the reference's formulation on torch device ops (F.batch_norm + F.relu; F.interpolate + F.cross_entropy +
torch.topk) on the same GPU in the same run, with the agreement of the results, and the fraction of the measured HBM
copy rate the norm passes reach.  No bar on time.  --out writes the same JSON to a file.

    python tools/bench_deeplab.py [--calls C] [--steps S] [--out profiles/deeplab_bench.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIG = os.path.join(ROOT, "tests", "golden", "configs", "deeplab_v3_plus_R_103_os16_mg124_poly_90k_bs16.yaml")
CL = torch.channels_last


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


def copy_rate(dev):
    """Bytes / s of a device-to-device copy of 1 GiB (read + write counted)."""
    a = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    ms = timed(lambda: b.copy_(a), 10)
    return 2.0 * a.numel() * 4 / (ms * 1e-3)


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def bench_norm(dev, calls, rate):
    from jtsm_amd.layers.batch_norm import BatchNorm2d
    g = torch.Generator().manual_seed(0)
    shape = (2, 256, 128, 256)
    x = torch.randn(*shape, generator=g).to(dev).contiguous(memory_format=CL).requires_grad_(True)
    dy = torch.randn(*shape, generator=g).to(dev).contiguous(memory_format=CL)
    ours, stock = BatchNorm2d(256).to(dev).train(), torch.nn.BatchNorm2d(256).to(dev).train()

    def run_ours():
        x.grad = None
        y = ours.fused(x, True)
        y.backward(dy)
        return y

    def run_stock():
        x.grad = None
        y = F.relu(stock(x))
        y.backward(dy)
        return y

    y0 = run_ours().detach().clone()
    g0 = x.grad.clone()
    y1 = run_stock().detach().clone()
    g1 = x.grad.clone()
    ms, ms_torch = timed(run_ours, calls), timed(run_stock, calls)
    n = x.numel()
    # forward: x read twice (statistics, apply), y written; backward: x, dy, y read twice, dx written
    moved = 4.0 * n * (3 + 7)
    return {"shape": list(shape), "ms": ms, "torch_ms": ms_torch, "output_agreement": rel(y0, y1),
            "dx_agreement": rel(g0, g1), "bytes": moved, "fraction_of_copy_rate": moved / (ms * 1e-3) / rate}


def bench_loss(dev, calls):
    from jtsm_amd.layers.elementwise import deeplab_cross_entropy
    g = torch.Generator().manual_seed(1)
    n, c, hs, ws, s = 2, 19, 128, 256, 4
    wide = (torch.randn(n, 20, hs, ws, generator=g) * 3).to(dev).contiguous(memory_format=CL).requires_grad_(True)
    target = torch.randint(0, c, (n, hs * s, ws * s), generator=g)
    target[torch.rand(n, hs * s, ws * s, generator=g) < 0.1] = 255
    target = target.to(dev)

    def run_ours():
        wide.grad = None
        loss = deeplab_cross_entropy(wide[:, :c], target, s, 255, 0.2)
        loss.backward()
        return loss

    def run_torch():
        wide.grad = None
        up = F.interpolate(wide[:, :c], scale_factor=s, mode="bilinear", align_corners=False)
        pl = F.cross_entropy(up, target, ignore_index=255, reduction="none").contiguous().view(-1)
        loss = torch.topk(pl, int(0.2 * pl.numel()))[0].mean()
        loss.backward()
        return loss

    l0 = run_ours().detach().clone()
    g0 = wide.grad.clone()
    l1 = run_torch().detach().clone()
    g1 = wide.grad.clone()
    return {"shape": [n, c, hs, ws, s], "ms": timed(run_ours, calls), "torch_ms": timed(run_torch, calls),
            "loss_agreement": rel(l0, l1), "dlogits_agreement": rel(g0, g1)}


def bench_step(dev, steps):
    from jtsm_amd.config import get_cfg
    from jtsm_amd.modeling import build_model
    from jtsm_amd.solver.build import build_optimizer
    cfg = get_cfg()
    cfg.merge_from_file(CONFIG)
    torch.manual_seed(0)
    model = build_model(cfg).train()
    opt = build_optimizer(cfg, model)
    g = torch.Generator().manual_seed(2)
    batch = []
    for _ in range(2):
        blocks = torch.randint(0, 19, (32, 64), generator=g)
        sem = blocks.repeat_interleave(16, 0).repeat_interleave(16, 1)
        sem[:, 500:524] = 255
        batch.append({"image": (torch.rand(3, 512, 1024, generator=g) * 255).to(dev), "sem_seg": sem.to(dev),
                      "height": 512, "width": 1024})
    last = {}

    def step():
        opt.zero_grad(set_to_none=True)
        losses = model(batch)
        sum(losses.values()).backward()
        opt.step()
        last["loss"] = losses["loss_sem_seg"].detach()

    ms = timed(step, steps)
    return {"config": os.path.basename(CONFIG), "input": [2, 3, 512, 1024], "ms_per_step": ms,
            "images_per_s": 2.0 / (ms * 1e-3), "loss_after": float(last["loss"]),
            "peak_memory_gib": torch.cuda.max_memory_allocated() / 2.0 ** 30}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_deeplab.py needs the MI355X"
    dev = torch.device("cuda:0")
    rate = copy_rate(dev)
    out = {"hbm_copy_rate_tb_s": rate / 1e12, "batch_norm_relu_fwd_bwd": bench_norm(dev, a.calls, rate),
           "hard_pixel_loss_fwd_bwd": bench_loss(dev, a.calls), "train_step": bench_step(dev, a.steps)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
