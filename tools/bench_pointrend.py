"""The PointRend operators alone.  Prints one JSON line, per call with wrapper, allocations and every launch included
(events around `--calls` calls after 3):

  train    the training point path at the shipped sizes — 2 images, a 256-channel p2 of 256 x 256 (1024 x 1024
           input), R = 128 foreground rois, 80 classes, 7 x 7 coarse logits, P = 196, oversampling 3, importance 0.75,
           eight 1024 x 1024 bitmasks per image: select + gather + loss, forward and backward into p2 and the coarse
           logits
  infer    the five-step subdivision at R = 100 on one image: 7 -> 224, N = 784

and, beside each, the reference's formulation written with torch device ops on the same GPU (the per-image
`grid_sample` loops, `topk`, index gathers, `interpolate` / `scatter_` over all 80 channels), with the agreement of the
results.  Both sides of these two share one stand-in point head, a single 336 -> 80 matmul, so that the operators
alone are compared.  Beside them `step`: the full training step (forward + backward, no optimiser) of the shipped
pointrend_rcnn_R_50_FPN_1x_coco config at 2 x 3 x 1024 x 1024 on synthetic inputs (jtsm_amd.utils.synthetic) with
three elliptic bitmask instances per image.  No bar on time.  --out writes the same JSON to a file.

    python tools/bench_pointrend.py [--calls C] [--out profiles/pointrend_bench.json]
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


def t_point_sample(x, pts):
    return F.grid_sample(x, 2.0 * pts.unsqueeze(2) - 1.0, align_corners=False).squeeze(3)


def t_wrt_image(boxes, pts):
    out = pts.clone()
    out[:, :, 0] = out[:, :, 0] * (boxes[:, None, 2] - boxes[:, None, 0]) + boxes[:, None, 0]
    out[:, :, 1] = out[:, :, 1] * (boxes[:, None, 3] - boxes[:, None, 1]) + boxes[:, None, 1]
    return out


def t_fine(feature, scale, boxes, counts, pts):
    """point_sample_fine_grained_features: one grid_sample per image on a one-image slice."""
    pim = t_wrt_image(boxes, pts)
    h, w = feature.shape[-2:]
    sc = torch.tensor([w, h], device=pts.device) / scale
    out = []
    for n, part in enumerate(torch.split(pim, counts)):
        out.append(t_point_sample(feature[n:n + 1], (part / sc).unsqueeze(0).flatten(1, 2)).view(
            feature.shape[1], part.shape[0], -1).transpose(0, 1))
    return torch.cat(out), pim


def t_select(coarse, classes, cand, rand, U):
    r = coarse.shape[0]
    logits = t_point_sample(coarse, cand)
    u = -logits[torch.arange(r, device=coarse.device), classes].abs()
    idx = torch.topk(u, U, dim=1)[1] + cand.shape[1] * torch.arange(r, device=coarse.device)[:, None]
    return torch.cat([cand.view(-1, 2)[idx.view(-1)].view(r, U, 2), rand], 1)


def t_loss(logits, classes, masks, counts, matched, pim):
    tgt = []
    for m, part, idx in zip(masks, torch.split(pim, counts), torch.split(matched, counts)):
        h, w = m.shape[-2:]
        sc = torch.tensor([w, h], dtype=torch.float, device=pim.device)
        tgt.append(t_point_sample(m[idx.long()].to(torch.float32).unsqueeze(1), part / sc).squeeze(1))
    r = logits.shape[0]
    return F.binary_cross_entropy_with_logits(logits[torch.arange(r, device=logits.device), classes], torch.cat(tgt))


def full_step_ms(steps, size=1024):
    from jtsm_amd.config import get_cfg
    from jtsm_amd.modeling import build_model
    from jtsm_amd.utils.synthetic import synthetic_inputs

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "tests", "golden", "configs", "pointrend_rcnn_R_50_FPN_1x_coco.yaml"))
    cfg.MODEL.DEVICE, cfg.MODEL.WEIGHTS = "cuda", ""
    torch.manual_seed(0)
    model = build_model(cfg)
    with torch.no_grad():
        model.backbone.bottom_up.stem.conv1.weight.mul_(1.0 / 64)
    data = []
    yy, xx = torch.meshgrid(torch.arange(size, device="cuda") + 0.5, torch.arange(size, device="cuda") + 0.5, indexing="ij")
    for d in synthetic_inputs(7, batch=2, size=size, proposals=8, n_things=3, num_things=80, device="cuda", keypoints=1):
        inst = d["instances"]
        inst.remove("gt_keypoints")
        b = inst.gt_boxes.tensor
        cx, cy, rx, ry = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, (b[:, 2] - b[:, 0]) / 2, (b[:, 3] - b[:, 1]) / 2
        inst.gt_masks = ((((xx[None] - cx[:, None, None]) / rx[:, None, None]) ** 2 +
                          ((yy[None] - cy[:, None, None]) / ry[:, None, None]) ** 2) <= 1).to(torch.uint8)
        data.append({"image": d["image"], "instances": inst})
    model.train()

    def step():
        model.zero_grad(set_to_none=True)
        sum(model(data).values()).backward()

    ms = timed(step, steps)
    del model
    torch.cuda.empty_cache()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from jtsm_amd.layers import point_rend as P

    dev = torch.device("cuda", 0)
    step_ms = full_step_ms(max(a.calls // 2, 5))
    rs = np.random.RandomState(7)
    torch.manual_seed(7)
    N, R, C, S, Pn, K, U = 2, 128, 80, 7, 196, 588, 147
    counts = [R // 2, R // 2]
    p2 = torch.randn(N, 256, 256, 256, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_()
    coarse = (2 * torch.randn(R, C, S, S, device=dev)).requires_grad_()
    x1, y1 = rs.uniform(0, 700, R), rs.uniform(0, 700, R)
    boxes = torch.from_numpy(np.stack([x1, y1, x1 + rs.uniform(32, 320, R), y1 + rs.uniform(32, 320, R)], 1)).float().to(dev)
    classes = torch.from_numpy(rs.randint(0, C, R)).to(dev)
    masks = [(torch.rand(8, 1024, 1024, device=dev) < 0.5).to(torch.uint8) for _ in range(N)]
    matched = torch.from_numpy(rs.randint(0, 8, R).astype(np.int32)).to(dev)
    roi_image = torch.repeat_interleave(torch.arange(N, dtype=torch.int32), torch.tensor(counts)).to(dev)
    head = (torch.randn(256 + C, C, device=dev) * 0.05).requires_grad_()
    cand, rand = torch.rand(R, K, 2, device=dev), torch.rand(R, Pn - U, 2, device=dev)

    def zero():
        p2.grad = coarse.grad = head.grad = None

    def ours_train():
        zero()
        pts = P.point_select(coarse, classes, cand, rand, Pn)
        rows, pim = P.point_gather([(p2, P.SHARED, 0.25, 0), (coarse, P.PER_ROI, 1.0, 256)], boxes, roi_image, pts)
        loss = P.point_loss(rows @ head, classes, masks, roi_image, matched, pim, Pn)
        loss.backward()
        return loss

    def torch_train():
        zero()
        with torch.no_grad():
            pts = t_select(coarse, classes, cand, rand, U)
        fine, pim = t_fine(p2, 0.25, boxes, counts, pts)
        feats = torch.cat([fine, t_point_sample(coarse, pts)], 1)                      # (R, 336, P)
        logits = torch.einsum("rcp,ck->rkp", feats, head)
        loss = t_loss(logits, classes, masks, counts, matched, pim)
        loss.backward()
        return loss

    train_ms, torch_train_ms = timed(ours_train, a.calls), timed(torch_train, a.calls)
    l0 = float(ours_train().detach())
    g0 = (p2.grad.clone(), coarse.grad.clone())
    l1 = float(torch_train().detach())
    g1 = (p2.grad.clone(), coarse.grad.clone())

    # ---- inference
    Ri, steps, Npts = 100, 5, 784
    p2i = p2.detach()[:1]
    ci, cls_i, bi = coarse.detach()[:Ri], classes[:Ri], boxes[:Ri]
    img_i = torch.zeros(Ri, dtype=torch.int32, device=dev)
    w = head.detach()

    def ours_infer():
        m = ci[torch.arange(Ri, device=dev), cls_i][:, None].contiguous()
        for step in range(steps):
            h, wd = m.shape[-2:]
            n = 0 if (Npts >= 16 * h * wd and step < steps - 1) else Npts
            m, idx, pts = P.point_subdivide(m, n)
            if n == 0:
                continue
            rows, _ = P.point_gather([(p2i, P.SHARED, 0.25, 0), (ci, P.PER_ROI, 1.0, 256)], bi, img_i, pts,
                                     want_coords=False)
            P.point_scatter(m, idx, rows @ w, cls_i)
        return m

    def torch_infer():
        m = ci.clone()
        for step in range(steps):
            m = F.interpolate(m, scale_factor=2, mode="bilinear", align_corners=False)
            h, wd = m.shape[-2:]
            if Npts >= 4 * h * wd and step < steps - 1:
                continue
            u = -m[torch.arange(Ri, device=dev), cls_i].abs()
            n = min(h * wd, Npts)
            idx = torch.topk(u.view(Ri, -1), n, dim=1)[1]
            pts = torch.stack([0.5 / wd + (idx % wd).float() / wd, 0.5 / h + (idx // wd).float() / h], -1)
            fine, _ = t_fine(p2i, 0.25, bi, [Ri], pts)
            feats = torch.cat([fine, t_point_sample(ci, pts)], 1)
            logits = torch.einsum("rcp,ck->rkp", feats, w)
            m = m.reshape(Ri, C, h * wd).scatter_(2, idx.unsqueeze(1).expand(-1, C, -1), logits).view(Ri, C, h, wd)
        return m[torch.arange(Ri, device=dev), cls_i][:, None]

    infer_ms, torch_infer_ms = timed(ours_infer, a.calls), timed(torch_infer, max(a.calls // 4, 2))
    m0, m1 = ours_infer(), torch_infer()
    close = float(((m0 - m1).abs() <= 1e-3).float().mean())

    out = {"workload": "train: 2 images, p2 256 x 256 x 256, R 128, C 80, P 196 (588 candidates), 8 bitmasks of 1024^2 per "
                       "image; infer: R 100, C 80, 7 -> 224 in five steps, N 784; stand-in point head = one 336 -> 80 matmul",
           "step_ms": round(step_ms, 3), "images_per_s": round(2 / step_ms * 1e3, 2),
           "step_workload": "pointrend_rcnn_R_50_FPN_1x_coco, 2 x 3 x 1024 x 1024, 3 elliptic bitmask instances per image",
           "train_point_path_fwd_bwd_ms_per_call": round(train_ms, 4),
           "torch_train_point_path_fwd_bwd_ms_per_call": round(torch_train_ms, 4),
           "train_loss_rel_diff": abs(l0 - l1) / abs(l1),
           "train_grad_p2_max_abs_diff": float((g0[0] - g1[0]).abs().max()),
           "train_grad_coarse_max_abs_diff": float((g0[1] - g1[1]).abs().max()),
           "subdivision_ms_per_call": round(infer_ms, 4), "torch_subdivision_ms_per_call": round(torch_infer_ms, 4),
           "subdivision_cells_within_1e-3": close, "calls": a.calls}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
