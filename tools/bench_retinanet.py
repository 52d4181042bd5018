"""RetinaNet at the benchmark size.  Prints one JSON line: ms per full training step (forward + backward, no optimiser)
and images / s of retinanet_R_50_FPN_1x (the flattened shipped configuration under tests/golden/configs/) at
2 x 3 x 1024 x 1024 on synthetic COCO-shaped ground truth, about 7 boxes per image; ms per call of the three fused
computations — anchor labelling, loss forward + backward, candidates + NMS — on the head's own outputs, wrapper,
allocations and every launch included (events around `--calls` calls after 3); beside each the same computation written
with torch device ops as the reference writes it, on the same GPU in the same run, with the agreement of the results;
and the bytes each fused call has to move against the measured HBM copy rate.  No bar on time.  --out writes the same
JSON to a file.

    python tools/bench_retinanet.py [--calls C] [--steps S] [--out profiles/retinanet_bench.json]
"""
import argparse
import json
import os
import sys

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


def synthetic_batch(n, size, boxes_per_image, num_classes, dev):
    from jtsm_amd.structures import Boxes, Instances
    g = torch.Generator().manual_seed(3)
    out = []
    for _ in range(n):
        k = boxes_per_image
        wh = torch.exp(torch.rand(k, 2, generator=g) * 3.0 + 3.0)                      # 20 .. 400 px, log-uniform
        x1y1 = torch.rand(k, 2, generator=g) * (size - wh).clamp(min=1)
        inst = Instances((size, size), gt_boxes=Boxes(torch.cat([x1y1, (x1y1 + wh).clamp(max=size)], 1)),
                         gt_classes=torch.randint(0, num_classes, (k,), generator=g))
        out.append({"image": (torch.rand(3, size, size, generator=g) * 255).to(dev), "instances": inst.to(dev),
                    "height": size, "width": size})
    return out


# ---- the reference's formulation on torch device ops ------------------------------------------------------------------
def torch_labels(model, anchors, gt_instances):
    from jtsm_amd.structures import Boxes, pairwise_iou
    flat = Boxes.cat(anchors)
    labels, boxes = [], []
    for g in gt_instances:
        idx, lab = model.anchor_matcher(pairwise_iou(g.gt_boxes, flat))
        out = g.gt_classes[idx]
        out[lab == 0] = model.num_classes
        out[lab == -1] = -1
        labels.append(out)
        boxes.append(g.gt_boxes.tensor[idx])
    return labels, boxes


def torch_losses(model, anchors, logits, deltas, gt_labels, gt_boxes, normalizer):
    k = model.num_classes
    labels = torch.stack(gt_labels)
    flat = type(anchors[0]).cat(anchors).tensor
    target = torch.stack([model.box2box_transform.get_deltas(flat, b) for b in gt_boxes])
    valid = labels >= 0
    pos = valid & (labels != k)
    num_pos = pos.sum().item()                                                       # the reference's read-back
    normalizer = 0.9 * normalizer + 0.1 * max(num_pos, 1)
    onehot = F.one_hot(labels[valid], num_classes=k + 1)[:, :-1]
    x = torch.cat(logits, dim=1)[valid]
    t = onehot.to(x.dtype)
    p = torch.sigmoid(x)
    ce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    p_t = p * t + (1 - p) * (1 - t)
    loss = ce * ((1 - p_t) ** model.focal_loss_gamma)
    loss = (model.focal_loss_alpha * t + (1 - model.focal_loss_alpha) * (1 - t)) * loss
    box = (torch.cat(deltas, dim=1)[pos] - target[pos]).abs().sum()                  # beta = 0: L1
    return loss.sum() / normalizer, box / normalizer


def torch_inference(model, anchors, logits, deltas, image_sizes):
    from jtsm_amd.layers.nms import batched_nms
    k = model.num_classes
    out = []
    for i in range(len(image_sizes)):
        boxes_all, scores_all, classes_all = [], [], []
        for x, d, a in zip(logits, deltas, anchors):
            prob = x[i].flatten().sigmoid()
            keep = prob > model.test_score_thresh
            prob, top = prob[keep], keep.nonzero().squeeze(1)
            prob, order = prob.sort(descending=True)
            n = min(model.test_topk_candidates, top.numel())
            prob, top = prob[:n], top[order[:n]]
            rows = top // k
            boxes_all.append(model.box2box_transform.apply_deltas(d[i][rows], a.tensor[rows]))
            scores_all.append(prob)
            classes_all.append(top % k)
        b, s, c = torch.cat(boxes_all), torch.cat(scores_all), torch.cat(classes_all)
        keep = batched_nms(b, s, c, model.test_nms_thresh)[:model.max_detections_per_image]
        out.append((b[keep], s[keep], c[keep]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from jtsm_amd.config import get_cfg
    from jtsm_amd.layers.retinanet import retinanet_candidates
    from jtsm_amd.modeling import build_model
    from jtsm_amd.modeling.meta_arch.retinanet import permute_to_N_HWA_K

    dev = torch.device("cuda", 0)
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "tests", "golden", "configs", "retinanet_R_50_FPN_1x.yaml"))
    cfg.MODEL.DEVICE = "cuda"
    torch.manual_seed(0)
    model = build_model(cfg)
    with torch.no_grad():
        model.backbone.bottom_up.stem.conv1.weight.mul_(1.0 / 64)
    n, k = 2, model.num_classes
    data = synthetic_batch(n, a.size, 7, k, dev)
    model.train()

    def step():
        model.zero_grad(set_to_none=True)
        sum(model(data).values()).backward()

    step_ms = timed(step, a.steps)

    # the head's outputs once, detached: what the three computations read
    with torch.no_grad():
        images = model.preprocess_image(data)
        feats = model.backbone(images.tensor)
        feats = [feats[f] for f in model.head_in_features]
        anchors = model.anchor_generator(feats)
        logits, deltas = model.head(feats)
    gt = [d["instances"] for d in data]
    r = sum(len(x) for x in anchors)

    label_ms = timed(lambda: model._label(anchors, gt), a.calls)
    torch_label_ms = timed(lambda: torch_labels(model, anchors, gt), a.calls)
    labels, matched, offsets, num_pos, gt_boxes = model._label(anchors, gt)
    t_labels, t_boxes = torch_labels(model, anchors, gt)
    labels_equal = bool(torch.equal(labels.long(), torch.stack(t_labels)))

    logits = [x.detach().requires_grad_() for x in logits]
    deltas = [x.detach().requires_grad_() for x in deltas]
    views = [permute_to_N_HWA_K(x, k) for x in logits], [permute_to_N_HWA_K(x, 4) for x in deltas]

    def clear():
        for t in logits + deltas:
            t.grad = None

    def ours():
        clear()
        model.loss_normalizer.fill_(100.0)
        sum(model._losses(anchors, logits, deltas, labels, matched, gt_boxes, offsets, num_pos).values()).backward()

    def theirs():
        clear()
        sum(torch_losses(model, anchors, views[0], views[1], t_labels, t_boxes, 100.0)).backward()

    loss_ms, torch_loss_ms = timed(ours, a.calls), timed(theirs, max(a.calls // 4, 2))
    ours()
    g0 = [t.grad.clone() for t in logits + deltas]
    model.loss_normalizer.fill_(100.0)
    l0 =[float(v.detach()) for v in model._losses(anchors, logits, deltas, labels, matched, gt_boxes, offsets, num_pos).values()]
    theirs()
    g1 = [t.grad.clone() for t in logits + deltas]
    l1 = [float(v.detach()) for v in torch_losses(model, anchors, views[0], views[1], t_labels, t_boxes, 100.0)]
    clear()

    model.eval()
    model.test_score_thresh = 0.005           # an untrained head scores every class near its prior 0.01: all pass
    with torch.no_grad():
        dl, dd = [x.detach() for x in logits], [x.detach() for x in deltas]
        dv = [permute_to_N_HWA_K(x, k) for x in dl], [permute_to_N_HWA_K(x, 4).contiguous() for x in dd]
        infer_ms = timed(lambda: model.inference(anchors, dl, dd, images.image_sizes), a.calls)
        flat = type(anchors[0]).cat(anchors).tensor
        cand_ms = timed(lambda: retinanet_candidates(dl, dd, flat, k, model.test_score_thresh,
                                                     model.test_topk_candidates), a.calls)
        torch_infer_ms = timed(lambda: torch_inference(model, anchors, dv[0], dv[1], images.image_sizes), max(a.calls // 4, 2))
        mine = model.inference(anchors, dl, dd, images.image_sizes)
        want = torch_inference(model, anchors, dv[0], dv[1], images.image_sizes)
    same = sum(int(len(m) == len(w[1]) and bool(torch.equal(m.pred_classes, w[2]))) for m, w in zip(mine, want))

    buf = torch.empty(64 << 20, dtype=torch.float32, device=dev)
    dst = torch.empty_like(buf)
    copy_ms = timed(lambda: dst.copy_(buf), 20)
    copy_gbs = 2 * buf.numel() * 4 / copy_ms / 1e6
    logit_bytes = n * r * k * 4
    # algorithmic bytes: labels read the anchors twice per image and write two ints per anchor; the loss reads the logits
    # once each way and writes their gradient; the candidates read the logits for two histograms and the compaction
    moved = {"label": n * r * (2 * 16 + 8), "loss_fwd_bwd": 3 * logit_bytes + 4 * n * r * 4, "candidates": 3 * logit_bytes}
    out = {"workload": "retinanet_R_50_FPN_1x, %d x 3 x %d x %d, 7 boxes per image, %d anchors per image, %d classes" % (n, a.size, a.size, r, k),
           "step_ms": round(step_ms, 3), "images_per_s": round(n / step_ms * 1e3, 2),
           "label_ms_per_call": round(label_ms, 4), "torch_label_ms_per_call": round(torch_label_ms, 4), "labels_equal": labels_equal,
           "loss_fwd_bwd_ms_per_call": round(loss_ms, 4), "torch_loss_fwd_bwd_ms_per_call": round(torch_loss_ms, 4),
           "loss_rel_diff": [abs(x - y) / max(abs(y), 1e-30) for x, y in zip(l0, l1)],
           "loss_grad_max_abs_diff": max(float((x - y).abs().max()) for x, y in zip(g0, g1)),
           "candidates_nms_ms_per_call": round(infer_ms, 4), "candidates_alone_ms_per_call": round(cand_ms, 4), "torch_candidates_nms_ms_per_call": round(torch_infer_ms, 4),
           "images_with_the_same_detection_classes": same, "score_thresh": model.test_score_thresh,
           "hbm_copy_GBps": round(copy_gbs, 1), "bytes_moved": moved,
           "fraction_of_copy_rate": {"label": round(moved["label"] / label_ms / 1e6 / copy_gbs, 4),
                                     "loss_fwd_bwd": round(moved["loss_fwd_bwd"] / loss_ms / 1e6 / copy_gbs, 4),
                                     "candidates": round(moved["candidates"] / cand_ms / 1e6 / copy_gbs, 4)},
           "calls": a.calls, "steps": a.steps}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
