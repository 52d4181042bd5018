"""ROILoopPool forward / backward on ContextLocNet's shipped shapes (512 channels, stride 8 on 1024 x 1024, 7 x 7 bins,
12 000 pooled rows), timed with hipEvents.  Prints one JSON line.

    python tools/bench_roi_loop_pool.py [--iters N]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from jtsm_amd.layers.roi_loop_pool import roi_loop_pool_backward, roi_loop_pool_forward
    from oracle import model as OM

    dev = torch.device("cuda:0")
    res = {}
    for name, B, R in (("B2_R2000", 2, 2000), ("B1_R4000", 1, 4000)):
        batch = OM.synthetic_batch(1234, B=B, size=1024, R=R, cluster=0.5)
        rois = torch.cat([torch.cat([torch.full((len(b), 1), float(i)), b], 1)
                          for i, b in enumerate(batch["boxes"])]).to(dev)
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(B, 512, 128, 128, device=dev, generator=g).clamp_(min=0).contiguous(
            memory_format=torch.channels_last)

        def timed(fn, n):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                r = fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n, r

        fwd, (out, arg) = timed(lambda: roi_loop_pool_forward(x, rois, 0.125, 7, 7), a.iters)
        gout = torch.randn_like(out)
        bwd, _ = timed(lambda: roi_loop_pool_backward(gout, rois, arg, 0.125, 7, 7, B, 512, 128, 128),
                       max(a.iters // 4, 1))
        written = 4 * (out.numel() + arg.numel())
        res[name] = dict(rows=int(out.shape[0]), fwd_ms=round(fwd, 4), out_bytes=4 * out.numel(),
                         written_bytes=written, fwd_TBps=round(written / fwd / 1e9, 3), bwd_ms=round(bwd, 3))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
