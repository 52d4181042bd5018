"""Panoptic-DeepLab at the benchmark size.  Prints one JSON line: ms per full training step (forward, backward and Adam)
and images / s of panoptic_deeplab_R_52_os16_mg124_poly_90k_bs32_crop_512_1024 (the flattened shipped configuration
under tests/golden/configs/) on 2 x 3 x 512 x 1024 synthetic crops with generated targets; and, per call with wrapper,
allocations and every launch included (events around `--calls` calls after 3),
  * the fused post-processing (arg-max, centres, grouping, merge, instance rows, one table copy) at 1024 x 2048 with
    about 30 instances,
  * the centre and the offset loss forward + backward at N = 2, 128 x 256 -> 512 x 1024,
  * one Adam step over the model's parameters,
each beside the reference's formulation on torch device ops on the same GPU in the same run (post_processing.py and the
instance loop of panoptic_seg.py restated with device tensors, host loops and `.item()` calls included; F.interpolate +
MSELoss / L1Loss; torch.optim.Adam), with the agreement of the results.  No bar on time.  --out writes the same JSON.

    python tools/bench_panoptic_deeplab.py [--calls C] [--steps S] [--out profiles/panoptic_deeplab_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIG = os.path.join(ROOT, "tests", "golden", "configs",
                      "panoptic_deeplab_R_52_os16_mg124_poly_90k_bs32_crop_512_1024.yaml")
CL = torch.channels_last
THINGS = tuple(range(11, 19))


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


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


# ---- post-processing ---------------------------------------------------------------------------------------------------
def scene(dev, h=1024, w=2048, instances=30):
    """19-class logits (eleven stuff bands, elliptic things of classes 11 .. 18), one heat peak per thing, offsets that
    point at the thing's centre plus noise."""
    g = torch.Generator().manual_seed(0)
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    cls = (xs * 11 // w).long()
    heat = torch.zeros(h, w)
    offsets = torch.randn(2, h, w, generator=g) * 2
    for k in range(instances):
        cy, cx = int(torch.randint(60, h - 60, (1,), generator=g)), int(torch.randint(80, w - 80, (1,), generator=g))
        ry, rx = int(torch.randint(30, 90, (1,), generator=g)), int(torch.randint(30, 120, (1,), generator=g))
        inside = ((ys - cy).float() / ry) ** 2 + ((xs - cx).float() / rx) ** 2 <= 1
        cls[inside] = 11 + k % 8
        heat = torch.maximum(heat, (0.95 - 0.01 * k) * torch.exp(-((ys - cy) ** 2 + (xs - cx) ** 2).float() / 128.0))
        offsets[0][inside] += (cy - ys[inside]).float()
        offsets[1][inside] += (cx - xs[inside]).float()
    logits = 4.0 * F.one_hot(cls, 19).permute(2, 0, 1).float() + torch.randn(19, h, w, generator=g)
    return logits.to(dev), heat.unsqueeze(0).to(dev), offsets.to(dev)


def torch_postprocess(logits, heat, offsets, label_divisor, stuff_area, threshold, nms_kernel, top_k):
    """The reference's path with device tensors: post_processing.get_panoptic_segmentation, then the instance loop of
    PanopticDeepLab.forward (np.unique on the host copy, one mask, mean and box per segment)."""
    sem = logits.argmax(dim=0, keepdim=True)
    thing_seg = torch.zeros_like(sem)
    for c in THINGS:
        thing_seg[sem == c] = 1
    x = F.threshold(heat, threshold, -1)
    pooled = F.max_pool2d(x, kernel_size=nms_kernel, stride=1, padding=(nms_kernel - 1) // 2)
    x = torch.where(x == pooled, x, torch.full_like(x, -1)).squeeze()
    kth = torch.topk(torch.flatten(x), top_k)[0][-1].clamp_(min=0)
    centers = torch.nonzero(x > kth)
    h, w = offsets.shape[1:]
    pan = torch.zeros_like(sem) - 1
    if centers.size(0) == 0:
        ins = torch.zeros_like(sem)
    else:
        yc, xc = torch.meshgrid(torch.arange(h, dtype=offsets.dtype, device=offsets.device),
                                torch.arange(w, dtype=offsets.dtype, device=offsets.device), indexing="ij")
        loc = (torch.stack([yc, xc]) + offsets).flatten(1).T.unsqueeze(0)
        distance = torch.norm(centers.unsqueeze(1) - loc, dim=-1)              # the K x HW intermediate
        ins = thing_seg * (torch.argmin(distance, dim=0).reshape(1, h, w) + 1)
    is_thing = (ins > 0) & (thing_seg > 0)
    counter = {}
    for i in torch.unique(ins):
        if i == 0:
            continue
        mask = (ins == i) & is_thing
        if torch.nonzero(mask).size(0) == 0:
            continue
        c = torch.mode(sem[mask].view(-1))[0].item()
        counter[c] = counter.get(c, 0) + 1
        pan[mask] = c * label_divisor + counter[c]
    for c in torch.unique(sem):
        if c.item() in THINGS:
            continue
        mask = (sem == c) & (ins == 0)
        if mask.sum().item() >= stuff_area:
            pan[mask] = c * label_divisor
    pan = pan.squeeze(0)
    prob = F.softmax(logits, dim=0)
    rows = []
    for label in np.unique(pan.cpu().numpy()):
        c = label // label_divisor
        if label == -1 or c not in THINGS:
            continue
        mask = pan == label
        score = torch.mean(prob[c][mask])
        idx = torch.nonzero(mask).float()
        cy, cx = torch.mean(idx[:, 0]), torch.mean(idx[:, 1])
        heat_at = heat[0, int(cy.item()), int(cx.item())]
        yy, xx = torch.nonzero(mask, as_tuple=True)
        rows.append(torch.stack([xx.min().float(), yy.min().float(), xx.max().float() + 1, yy.max().float() + 1,
                                 score, heat_at]))
    return pan, torch.stack(rows) if rows else torch.zeros(0, 6, device=pan.device)


def bench_postprocess(dev, calls):
    from jtsm_amd.layers.panoptic_deeplab import panoptic_deeplab_postprocess
    logits, heat, offsets = scene(dev)
    args = (1000, 2048, 0.1, 7, 200)

    def ours():
        return panoptic_deeplab_postprocess(logits, heat, offsets, THINGS, args[0], args[1], args[2], args[3], args[4],
                                            void_label=-1, id_offset=0)

    def stock():
        return torch_postprocess(logits, heat.clone(), offsets, *args)

    a, (pan, rows) = ours(), stock()
    same = int((a["panoptic"].long() != pan).sum())
    inst = a["instances"]
    order = torch.argsort(a["table"][:inst.shape[0], 0])          # the torch form lists segments by ascending id
    agree = {"pixels_that_differ": same, "thing_segments": int(inst.shape[0]), "torch_thing_segments": int(rows.shape[0])}
    if inst.shape[0] == rows.shape[0] and inst.shape[0] > 0:
        agree["boxes_equal"] = bool(torch.equal(inst[order, :4], rows[:, :4]))
        agree["semantic_score_agreement"] = rel(inst[order, 4], rows[:, 4])
        agree["centre_score_equal"] = bool(torch.equal(inst[order, 5], rows[:, 5]))
    return {"shape": [19, 1024, 2048], "centres": int(a["num_centers"]), "ms": timed(ours, calls),
            "torch_ms": timed(stock, max(2, calls // 4)), **agree}


# ---- losses ------------------------------------------------------------------------------------------------------------
def bench_losses(dev, calls):
    from jtsm_amd.layers.panoptic_deeplab import center_loss, offset_loss
    g = torch.Generator().manual_seed(1)
    n, hs, ws, s = 2, 128, 256, 4
    out = {}
    for name, c, fn in (("center", 1, center_loss), ("offset", 2, offset_loss)):
        wide = torch.randn(n, 8, hs, ws, generator=g).to(dev).contiguous(memory_format=CL).requires_grad_(True)
        target = (torch.randn(n, c, hs * s, ws * s, generator=g) * (10 if c == 2 else 1)).to(dev)
        weights = (torch.rand(n, 1, hs * s, ws * s, generator=g) < 0.6).float().to(dev)

        def ours():
            wide.grad = None
            loss = fn(wide[:, :c], target, weights, s)
            loss.backward()
            return loss

        def stock():
            wide.grad = None
            up = F.interpolate(wide[:, :c], scale_factor=s, mode="bilinear", align_corners=False)
            if c == 1:
                loss = F.mse_loss(up, target, reduction="none") * weights
            else:
                loss = F.l1_loss(up * s, target, reduction="none") * weights
            loss = loss.sum() / weights.sum() if weights.sum() > 0 else loss.sum() * 0      # (the host synchronisation)
            loss.backward()
            return loss

        l0 = ours().detach().clone()
        g0 = wide.grad.clone()
        l1 = stock().detach().clone()
        g1 = wide.grad.clone()
        out[name + "_loss_fwd_bwd"] = {"shape": [n, c, hs, ws, s], "ms": timed(ours, calls), "torch_ms": timed(stock, calls),
                                       "loss_agreement": rel(l0, l1), "gradient_agreement": rel(g0[:, :c], g1[:, :c])}
    return out


# ---- the model: Adam alone, and the full step ------------------------------------------------------------------------
def batch_of(cfg, dev):
    from jtsm_amd.data import PanopticDeepLabTargetGenerator
    gen = PanopticDeepLabTargetGenerator(cfg.MODEL.SEM_SEG_HEAD.IGNORE_VALUE, THINGS, sigma=cfg.INPUT.GAUSSIAN_SIGMA,
                                         ignore_stuff_in_offset=cfg.INPUT.IGNORE_STUFF_IN_OFFSET,
                                         small_instance_area=cfg.INPUT.SMALL_INSTANCE_AREA,
                                         small_instance_weight=cfg.INPUT.SMALL_INSTANCE_WEIGHT,
                                         ignore_crowd_in_semantic=cfg.INPUT.IGNORE_CROWD_IN_SEMANTIC)
    g = torch.Generator().manual_seed(2)
    ys, xs = np.mgrid[:512, :1024]
    batch = []
    for _ in range(2):
        pan = (xs * 10 // 1024 + 1).astype(np.int32)
        pan[:, 500:524] = 0
        segments = [dict(id=i + 1, category_id=i, iscrowd=0) for i in range(10)]
        for k in range(8):
            cy, cx = int(torch.randint(40, 470, (1,), generator=g)), int(torch.randint(60, 960, (1,), generator=g))
            pan[((ys - cy) / 35.0) ** 2 + ((xs - cx) / 50.0) ** 2 <= 1] = 100 + k
            segments.append(dict(id=100 + k, category_id=11 + k, iscrowd=0))
        item = {"image": (torch.rand(3, 512, 1024, generator=g) * 255).to(dev), "height": 512, "width": 1024}
        item.update({k: v.to(dev) for k, v in gen(pan, segments).items() if k != "center_points"})
        batch.append(item)
    return batch


def bench_model(dev, steps, calls):
    from jtsm_amd.config import add_panoptic_deeplab_config, get_cfg
    from jtsm_amd.modeling import build_model
    from jtsm_amd.solver.build import build_optimizer
    cfg = get_cfg()
    add_panoptic_deeplab_config(cfg)
    cfg.merge_from_file(CONFIG)
    torch.manual_seed(0)
    model = build_model(cfg).train()
    opt = build_optimizer(cfg, model)
    batch = batch_of(cfg, dev)
    last = {}

    def step():
        opt.zero_grad(set_to_none=True)
        losses = model(batch)
        sum(losses.values()).backward()
        opt.step()
        last.update({k: float(v.detach()) for k, v in losses.items()})

    ms = timed(step, steps)
    peak = torch.cuda.max_memory_allocated() / 2.0 ** 30
    # Adam alone, on the gradients the last step left, beside torch.optim.Adam over clones of the same tensors
    opt.zero_grad(set_to_none=True)
    sum(model(batch).values()).backward()
    params = [p for p in model.parameters() if p.grad is not None]
    twins = [p.detach().clone().requires_grad_(True) for p in params]
    for t, p in zip(twins, params):
        t.grad = p.grad.clone()
    stock = torch.optim.Adam(twins, lr=cfg.SOLVER.BASE_LR)
    adam = {"parameters": len(params), "elements": int(sum(p.numel() for p in params)),
            "ms": timed(opt.step, calls), "torch_ms": timed(stock.step, calls)}
    return ({"config": os.path.basename(CONFIG), "input": [2, 3, 512, 1024], "ms_per_step": ms,
             "images_per_s": 2.0 / (ms * 1e-3), "losses_after": last, "peak_memory_gib": peak}, adam)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_panoptic_deeplab.py needs the MI355X"
    dev = torch.device("cuda:0")
    out = {"postprocess": bench_postprocess(dev, a.calls)}
    out.update(bench_losses(dev, a.calls))
    out["train_step"], out["adam_step"] = bench_model(dev, a.steps, a.calls)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
