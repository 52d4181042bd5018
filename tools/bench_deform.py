"""Deformable convolution beside the plain 3x3 at the backbone's shapes.  Prints one JSON line; --out writes it to a file.

    python tools/bench_deform.py [--calls C] [--rounds R] [--out profiles/deform_bench.json]

N = 2 images of 1024 x 1024: the R50-FPN res3 / res4 / res5 3x3 shapes (C = 128 at 128 x 128, 256 at 64 x 64, 512 at
32 x 32) and the DC5 res5 shape (C = 512 at 64 x 64, dilation 2); stride 1, O = C, one deformable group, offsets uniform
in [-2, 2], mask uniform in [0, 1].  Per shape:

* forward + backward (gradients of the input, the weight, the offsets and the mask) of `DeformConv`, of
  `ModulatedDeformConv` and, as a yardstick, of this package's own plain 3x3 `conv2d_fused` on the same input and weight.
  The three are timed in turn, `--rounds` times, `--calls` calls per turn after a warm-up; the figure is the median turn,
  with the fastest and slowest turn beside it (the box's spread).
* the three kernels alone (columns; offset / mask gradient; input gradient with its key, sort, segment and walk stages),
  device events around `--calls` calls, with the bytes each must move (computed from the shapes below) over that time
  beside the rate of a device-to-device copy of 256 MiB measured in the same process.
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("res3", 128, 128, 128, 1), ("res4", 256, 64, 64, 1), ("res5", 512, 32, 32, 1), ("dc5_res5", 512, 64, 64, 2)]
N, K, G = 2, 9, 1


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


def spread(turns):
    return {"ms": round(statistics.median(turns), 4), "min_ms": round(min(turns), 4), "max_ms": round(max(turns), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deform.py needs the MI355X")
    from jtsm_amd.layers import DeformConv, ModulatedDeformConv
    from jtsm_amd.layers import conv as CV
    D = importlib.import_module("jtsm_amd.layers.deform_conv")

    dev = torch.device("cuda", 0)
    CL = torch.channels_last
    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    copy_ms = timed(lambda: dst.copy_(src), a.calls)
    copy_gbs = 2 * src.numel() / copy_ms * 1e-6
    del src, dst
    out = {"workload": "N = 2, 1024 x 1024 input: 3x3 deformable conv v1 / v2 at the R50-FPN and DC5 shapes, forward + "
                       "backward, offsets uniform in [-2, 2], beside the plain 3x3 conv2d_fused",
           "conv_math": CV.MATH, "calls": a.calls, "rounds": a.rounds, "hbm_copy_GBps": round(copy_gbs, 1), "shapes": {}}
    for name, C, H, W, dil in SHAPES:
        g = torch.Generator().manual_seed(C + H)
        x = torch.randn(N, C, H, W, generator=g).to(dev).contiguous(memory_format=CL).requires_grad_()
        offset = (torch.rand(N, 2 * K * G, H, W, generator=g) * 4 - 2).to(dev).contiguous(memory_format=CL).requires_grad_()
        mask = torch.rand(N, K * G, H, W, generator=g).to(dev).contiguous(memory_format=CL).requires_grad_()
        dy = torch.randn(N, C, H, W, generator=g).to(dev).contiguous(memory_format=CL)
        v1 = DeformConv(C, C, 3, 1, dil, dil, 1, G).to(dev)
        v2 = ModulatedDeformConv(C, C, 3, 1, dil, dil, 1, G, bias=False).to(dev)
        with torch.no_grad():
            v2.weight.copy_(v1.weight)

        def step(forward, params):
            def run():
                CV.planes_clear()
                for t in params:
                    t.grad = None
                forward().backward(dy)
            return run

        runs = {"deform_v1": step(lambda: v1(x, offset), [x, offset, v1.weight]),
                "deform_v2": step(lambda: v2(x, offset, mask), [x, offset, mask, v2.weight]),
                "plain_3x3": step(lambda: CV.conv2d_fused(x, v1.weight, stride=1, pad=dil, dil=dil), [x, v1.weight])}
        turns = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                turns[k].append(timed(fn, a.calls))
        row = {k: spread(v) for k, v in turns.items()}
        for k in ("deform_v1", "deform_v2"):
            row[k]["times_plain"] = round(row[k]["ms"] / row["plain_3x3"]["ms"], 2)
        # the kernels alone (v2: with the mask)
        xd, od, md = x.detach(), offset.detach(), mask.detach()
        geo = dict(kh=3, kw=3, stride=1, pad=dil, dil=dil, G=G)
        cols = D.deform_columns(xd, od, md, **geo)
        dcols = torch.randn_like(cols)
        f = 4.0          # bytes per element
        col_bytes, x_bytes = f * cols.numel(), f * xd.numel()
        aux = f * (od.numel() + md.numel())
        kernels = {
            "columns": (lambda: D.deform_columns(xd, od, md, out=cols, **geo), x_bytes + aux + col_bytes),
            "offset_mask_grad": (lambda: D.deform_offset_mask_grad(dcols, xd, od, md, **geo), col_bytes + x_bytes + 2 * aux),
            "input_grad": (lambda: D.deform_input_grad(dcols, od, md, xd.shape, **geo), col_bytes + aux + x_bytes)}
        row["kernels"] = {}
        for k, (fn, nbytes) in kernels.items():
            ms = statistics.median(timed(fn, a.calls) for _ in range(3))
            row["kernels"][k] = {"ms": round(ms, 4), "MB": round(nbytes * 1e-6, 1), "GBps": round(nbytes / ms * 1e-6, 1),
                                 "of_copy_rate": round(nbytes / ms * 1e-6 / copy_gbs, 3)}
        row["input_grad_workspace_MB"] = round(CV.L.lib().jtsm_deform_input_grad_workspace_bytes(N, H, W, G, 3, 3, 1, dil, dil)
                                               * 1e-6, 1)
        row["shape"] = {"N": N, "C": C, "H": H, "W": W, "dilation": dil}
        out["shapes"][name] = row
        del cols, dcols
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f_:
            f_.write(line + "\n")


if __name__ == "__main__":
    main()
