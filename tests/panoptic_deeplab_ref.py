"""Panoptic-DeepLab restated with stock torch / NumPy CPU ops: the post-processing (find_instance_center, group_pixels,
merge_semantic_and_instance, get_panoptic_segmentation), the instance rows, the centre / offset losses and the target
generator of projects/Panoptic-DeepLab/panoptic_deeplab/.  tests/golden/panoptic_deeplab.npz holds what the reference's
own post_processing.py and target_generator.py gave for the inputs built here (tools/make_panoptic_deeplab_golden.py);
tests/test_panoptic_deeplab_ref.py pins this file to those vectors bit for bit, and the GPU tests compare the kernels
with this file."""
import numpy as np
import torch
import torch.nn.functional as F


# ---- post-processing ---------------------------------------------------------------------------------------------------
def find_instance_center(center_heatmap, threshold=0.1, nms_kernel=3, top_k=None):
    """(1,H,W) heat -> (K,2) int64 (y, x), torch.nonzero's order."""
    x = F.threshold(center_heatmap.clone(), threshold, -1)
    pooled = F.max_pool2d(x, kernel_size=nms_kernel, stride=1, padding=(nms_kernel - 1) // 2)
    x = torch.where(x == pooled, x, torch.full_like(x, -1)).squeeze()
    assert x.dim() == 2
    if top_k is None:
        return torch.nonzero(x > 0)
    kth = torch.topk(x.flatten(), top_k).values[-1].clamp(min=0)
    return torch.nonzero(x > kth)


def center_distances(center_points, offsets, dtype=None):
    """(K, H*W) distances of every pixel's voted location to every centre, in offsets' dtype (or `dtype`)."""
    if dtype is not None:
        offsets = offsets.to(dtype)
    h, w = offsets.shape[1:]
    ys = torch.arange(h, dtype=offsets.dtype).view(h, 1).expand(h, w)
    xs = torch.arange(w, dtype=offsets.dtype).view(1, w).expand(h, w)
    loc = (torch.stack([ys, xs]) + offsets).flatten(1).T.unsqueeze(0)          # (1, HW, 2)
    return torch.norm(center_points.unsqueeze(1) - loc, dim=-1)


def group_pixels(center_points, offsets):
    """-> (1,H,W) int64 in [1, K]."""
    h, w = offsets.shape[1:]
    return torch.argmin(center_distances(center_points, offsets), dim=0).reshape(1, h, w) + 1


def thing_mask(sem_seg, thing_ids):
    out = torch.zeros_like(sem_seg)
    for c in thing_ids:
        out[sem_seg == c] = 1
    return out


def merge_semantic_and_instance(sem_seg, ins_seg, thing_seg, label_divisor, thing_ids, stuff_area, void_label,
                                id_offset=0):
    """-> (pan (1,H,W), table rows [[id, isthing, category, instance_id, area] ...]): things in ascending instance
    order, then stuff in ascending class order; every id (and void) + id_offset."""
    pan = torch.zeros_like(sem_seg) + void_label
    is_thing = (ins_seg > 0) & (thing_seg > 0)
    rows, counter = [], {}
    for i in torch.unique(ins_seg).tolist():
        if i == 0:
            continue
        mask = (ins_seg == i) & is_thing
        area = int(mask.sum())
        if area == 0:
            continue
        cls = int(torch.mode(sem_seg[mask].view(-1))[0])
        counter[cls] = counter.get(cls, 0) + 1
        pan[mask] = cls * label_divisor + counter[cls]
        rows.append([cls * label_divisor + counter[cls] + id_offset, 1, cls, counter[cls], area])
    for cls in torch.unique(sem_seg).tolist():
        if cls in thing_ids:
            continue
        mask = (sem_seg == cls) & (ins_seg == 0)
        area = int(mask.sum())
        if area >= stuff_area:
            pan[mask] = cls * label_divisor
            rows.append([cls * label_divisor + id_offset, 0, cls, -1, area])
    return pan + id_offset, rows


def get_panoptic_segmentation(sem_seg, center_heatmap, offsets, thing_ids, label_divisor, stuff_area, void_label,
                              threshold=0.1, nms_kernel=7, top_k=200, id_offset=0):
    """-> (pan (1,H,W) int64, centers (1,K,2), table rows)."""
    thing_seg = thing_mask(sem_seg, thing_ids)
    centers = find_instance_center(center_heatmap, threshold, nms_kernel, top_k)
    if centers.size(0) == 0:
        ins = torch.zeros_like(sem_seg)
    else:
        ins = thing_seg * group_pixels(centers, offsets)
    pan, rows = merge_semantic_and_instance(sem_seg, ins, thing_seg, label_divisor, thing_ids, stuff_area, void_label,
                                            id_offset)
    return pan, centers.unsqueeze(0), rows


def instance_rows(pan, rows, logits, heat, dtype):
    """Per thing row {x0, y0, x1 + 1, y1 + 1, mean soft-max probability of its class, centre heat, centre y, centre x}.
    dtype float64: exact coordinate means (integer sums divided in fp64) and an fp64 soft-max; float32: the reference's
    formulation (panoptic_seg.py:187-199: fp32 soft-max, torch.mean of the masked values and of the float indices)."""
    pan = pan.reshape(pan.shape[-2:])
    prob = F.softmax(logits.to(dtype), dim=0)
    out = []
    for sid, isthing, cls, _, area in rows:
        if not isthing:
            continue
        mask = pan == sid
        idx = torch.nonzero(mask)
        if dtype == torch.float64:
            cy, cx = int(int(idx[:, 0].sum()) / area), int(int(idx[:, 1].sum()) / area)
        else:
            f = idx.float()
            cy, cx = int(torch.mean(f[:, 0]).item()), int(torch.mean(f[:, 1]).item())
        out.append([float(idx[:, 1].min()), float(idx[:, 0].min()), float(idx[:, 1].max() + 1), float(idx[:, 0].max() + 1),
                    float(torch.mean(prob[cls][mask])), float(heat.reshape(pan.shape)[cy, cx]), float(cy), float(cx)])
    return torch.tensor(out, dtype=torch.float64).reshape(-1, 8)


# ---- losses ------------------------------------------------------------------------------------------------------------
def _weighted_mean(loss, weights):
    total = weights.sum()
    return loss.sum() / total if total > 0 else loss.sum() * 0


def center_loss(pred, target, weights, scale, dtype=torch.float64):
    up = F.interpolate(pred.to(dtype), scale_factor=scale, mode="bilinear", align_corners=False)
    return _weighted_mean(F.mse_loss(up, target.to(dtype), reduction="none") * weights.to(dtype), weights.to(dtype))


def offset_loss(pred, target, weights, scale, dtype=torch.float64):
    up = F.interpolate(pred.to(dtype), scale_factor=scale, mode="bilinear", align_corners=False) * scale
    return _weighted_mean(F.l1_loss(up, target.to(dtype), reduction="none") * weights.to(dtype), weights.to(dtype))


def loss_and_grad(fn, pred, target, weights, scale, dtype):
    p = pred.detach().clone().to(dtype).requires_grad_(True)
    loss = fn(p, target, weights, scale, dtype)
    loss.backward()
    return loss.detach(), p.grad


# ---- target generator --------------------------------------------------------------------------------------------------
def generate_targets(panoptic, segments_info, ignore_label, thing_ids, sigma=8, ignore_stuff_in_offset=False,
                     small_instance_area=0, small_instance_weight=1, ignore_crowd_in_semantic=False):
    """The seven targets as NumPy arrays: sem_seg int64, center, offset, sem_seg_weights, center_weights,
    offset_weights float32, center_points (P,2) float64."""
    h, w = panoptic.shape
    size = 6 * sigma + 3
    t = np.arange(0, size, 1, float)
    gauss = np.exp(-((t - (3 * sigma + 1)) ** 2 + (t[:, None] - (3 * sigma + 1)) ** 2) / (2 * sigma ** 2))
    sem = np.full((h, w), ignore_label, np.uint8)
    center, offset = np.zeros((h, w), np.float32), np.zeros((2, h, w), np.float32)
    sem_w = np.ones((h, w), np.uint8)
    cen_w, off_w = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    points = []
    for seg in segments_info:
        m, cat = panoptic == seg["id"], seg["category_id"]
        if not (ignore_crowd_in_semantic and seg["iscrowd"]):
            sem[m] = cat
        if not seg["iscrowd"]:
            cen_w[m] = 1
            if cat in thing_ids or not ignore_stuff_in_offset:
                off_w[m] = 1
        if cat not in thing_ids or not m.any():
            continue
        rows, cols = np.where(m)
        if len(rows) < small_instance_area:
            sem_w[m] = small_instance_weight
        cy, cx = np.mean(rows), np.mean(cols)
        points.append([cy, cx])
        y, x = int(round(cy)), int(round(cx))
        x_lo, y_lo = int(np.round(x - 3 * sigma - 1)), int(np.round(y - 3 * sigma - 1))
        x_hi, y_hi = int(np.round(x + 3 * sigma + 2)), int(np.round(y + 3 * sigma + 2))
        ax, bx, ay, by = max(0, x_lo), min(x_hi, w), max(0, y_lo), min(y_hi, h)
        center[ay:by, ax:bx] = np.maximum(center[ay:by, ax:bx], gauss[ay - y_lo:by - y_lo, ax - x_lo:bx - x_lo])
        offset[0][rows, cols] = cy - yy[rows, cols]
        offset[1][rows, cols] = cx - xx[rows, cols]
    return dict(sem_seg=sem.astype(np.int64), center=center, offset=offset, sem_seg_weights=sem_w.astype(np.float32),
                center_weights=cen_w[None].astype(np.float32), offset_weights=off_w[None].astype(np.float32),
                center_points=np.asarray(points, np.float64).reshape(-1, 2))


# ---- the inputs of the golden file ------------------------------------------------------------------------------------
SCENE = dict(thing_ids=(4, 5, 6), num_classes=7, label_divisor=100, stuff_area=600, void_label=-1, threshold=0.1,
             nms_kernel=7, top_k=20)
TARGETS = dict(ignore_label=255, thing_ids=(3, 4), sigma=3, ignore_stuff_in_offset=True, small_instance_area=60,
               small_instance_weight=3, ignore_crowd_in_semantic=True)


def synthetic_scene(seed=0, h=48, w=64):
    """Three stuff stripes (classes 0, 1, 2; the last below stuff_area once the things are taken out), a corner patch of
    stuff class 3 (void: too small), five elliptic things of classes 4, 5, 6 (two of one class; one whose left third
    votes for another class), a centre heat map with one peak per thing, offsets that point at the thing's centre plus
    noise.  Every value sits on a coarse binary grid (logits 1/8, heat 1/1024, offsets 1/4), so the file compresses
    and the fp32 distances are exact.  -> logits (C,H,W), heat (1,H,W), offsets (2,H,W) float32."""
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    cls = torch.zeros(h, w, dtype=torch.int64)
    cls[20:40] = 1
    cls[40:] = 2
    cls[:5, :6] = 3
    things = [(10, 14, 6, 9, 4), (12, 44, 7, 8, 5), (30, 20, 6, 10, 4), (33, 50, 8, 7, 6), (43, 30, 4, 12, 5)]
    heat = torch.zeros(h, w)
    offsets = torch.zeros(2, h, w)
    for k, (cy, cx, ry, rx, c) in enumerate(things):
        inside = ((ys - cy).float() / ry) ** 2 + ((xs - cx).float() / rx) ** 2 <= 1
        cls[inside] = c
        if k == 2:
            cls[inside & (xs < cx - rx // 3)] = 5
        heat = torch.maximum(heat, (0.9 - 0.1 * k) * torch.exp(-((ys - cy) ** 2 + (xs - cx) ** 2).float() / 8.0))
        offsets[0][inside] = (cy - ys[inside]).float()
        offsets[1][inside] = (cx - xs[inside]).float()
    offsets = offsets + torch.randint(-6, 7, (2, h, w), generator=g).float() / 4
    heat = torch.round((heat + 0.05 * torch.rand(h, w, generator=g)) * 1024) / 1024
    logits = 4.0 * F.one_hot(cls, 7).permute(2, 0, 1).float() + torch.randint(-8, 9, (7, h, w), generator=g).float() / 8
    return logits, heat.unsqueeze(0), offsets


def target_scene():
    """A (40,56) panoptic map and its segments: two stuff segments, a thing near the border (clipped Gaussian), a small
    thing (semantic weight 3), a crowd thing, an unlabelled band, and a segment that has no pixel."""
    pan = np.zeros((40, 56), np.int32)
    pan[:18] = 7
    pan[18:36] = 8
    ys, xs = np.mgrid[:40, :56]
    pan[((ys - 3) / 6.0) ** 2 + ((xs - 50) / 9.0) ** 2 <= 1] = 3001
    pan[((ys - 24) / 3.0) ** 2 + ((xs - 12) / 4.0) ** 2 <= 1] = 3002
    pan[((ys - 26) / 7.0) ** 2 + ((xs - 36) / 8.0) ** 2 <= 1] = 4001
    pan[10:16, 20:34] = 4002
    segments = [dict(id=7, category_id=0, iscrowd=0), dict(id=8, category_id=1, iscrowd=0),
                dict(id=3001, category_id=3, iscrowd=0), dict(id=3002, category_id=3, iscrowd=0),
                dict(id=4001, category_id=4, iscrowd=0), dict(id=4002, category_id=4, iscrowd=1),
                dict(id=4003, category_id=4, iscrowd=0)]
    return pan, segments
