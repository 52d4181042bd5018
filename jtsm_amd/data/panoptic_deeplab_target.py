"""PanopticDeepLabTargetGenerator — the training targets of Panoptic-DeepLab from a panoptic label map: what
projects/Panoptic-DeepLab/panoptic_deeplab/target_generator.py computes, written from its behaviour.  Host NumPy, as the
data layer of this package is host code.  The number formats of every step are part of the behaviour, because they
decide the bits: the Gaussian template and an instance's mean row / column are fp64, the heat map and the offsets are
fp32 arrays those fp64 values are rounded into, and the coordinate grids are fp32."""
import numpy as np
import torch


def _gaussian_template(sigma):
    """(6 sigma + 3)^2 fp64 template exp(-(dx^2 + dy^2) / (2 sigma^2)) whose peak, 1, sits at index 3 sigma + 1."""
    t = np.arange(0, 6 * sigma + 3, 1, float) - (3 * sigma + 1)
    return np.exp(-(t[None, :] ** 2 + t[:, None] ** 2) / (2 * sigma ** 2))


class PanopticDeepLabTargetGenerator(object):
    """Callable with the reference's constructor keywords.  ignore_label: label of unannotated pixels; thing_ids:
    contiguous ids of the thing classes; sigma: of the centre Gaussian; ignore_stuff_in_offset: the offset loss skips
    stuff; small_instance_area / small_instance_weight: thing segments with fewer pixels get this semantic loss weight;
    ignore_crowd_in_semantic: crowd segments keep the ignore label."""

    def __init__(self, ignore_label, thing_ids, sigma=8, ignore_stuff_in_offset=False, small_instance_area=0,
                 small_instance_weight=1, ignore_crowd_in_semantic=False):
        self.ignore_label, self.thing_ids, self.sigma = ignore_label, set(thing_ids), sigma
        self.ignore_stuff_in_offset, self.ignore_crowd_in_semantic = ignore_stuff_in_offset, ignore_crowd_in_semantic
        self.small_instance_area, self.small_instance_weight = small_instance_area, small_instance_weight
        self.g = _gaussian_template(sigma)

    def _stamp(self, heat, cy, cx):
        """Element-wise maximum of `heat` and the template with its peak at the rounded (cy, cx), clipped to the map."""
        h, w = heat.shape
        reach = 3 * self.sigma + 1
        top, left = int(np.round(int(round(cy)) - reach)), int(np.round(int(round(cx)) - reach))
        size = self.g.shape[0]
        r0, r1, c0, c1 = max(top, 0), min(top + size, h), max(left, 0), min(left + size, w)
        window = heat[r0:r1, c0:c1]
        np.maximum(window, self.g[r0 - top:r1 - top, c0 - left:c1 - left], out=window)

    def __call__(self, panoptic, segments_info):
        """panoptic: (H,W) integer segment ids; segments_info: dicts with id, category_id, iscrowd.  Returns a dict:
        sem_seg (H,W) int64; center (H,W) float32 heat; center_points, a list of [y, x] fp64 means, one per thing segment
        that has a pixel; offset (2,H,W) float32 (to the centre, y then x); sem_seg_weights (H,W), center_weights and
        offset_weights (1,H,W) float32."""
        h, w = panoptic.shape[:2]
        labels = np.full((h, w), self.ignore_label, np.uint8)
        loss_w = np.ones((h, w), np.uint8)
        in_center, in_offset = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
        heat = np.zeros((h, w), np.float32)
        votes = np.zeros((2, h, w), np.float32)
        rows_f = np.arange(h, dtype=np.float32)[:, None].repeat(w, 1)
        cols_f = np.arange(w, dtype=np.float32)[None, :].repeat(h, 0)
        points = []
        for seg in segments_info:
            region = panoptic == seg["id"]
            cat, crowd = seg["category_id"], bool(seg["iscrowd"])
            thing = cat in self.thing_ids
            if not (crowd and self.ignore_crowd_in_semantic):
                labels[region] = cat
            if not crowd:                   # unlabelled pixels and crowds train neither instance branch
                in_center[region] = 1
                if thing or not self.ignore_stuff_in_offset:
                    in_offset[region] = 1
            if not thing or not region.any():       # (a segment may have been cropped away entirely)
                continue
            ys, xs = np.nonzero(region)
            if ys.size < self.small_instance_area:
                loss_w[region] = self.small_instance_weight
            cy, cx = ys.mean(), xs.mean()           # fp64
            points.append([cy, cx])
            self._stamp(heat, cy, cx)
            votes[0][ys, xs] = cy - rows_f[ys, xs]
            votes[1][ys, xs] = cx - cols_f[ys, xs]
        as_f32 = lambda a: torch.as_tensor(a.astype(np.float32))  # noqa: E731
        return {"sem_seg": torch.as_tensor(labels.astype(np.int64)), "center": as_f32(heat), "center_points": points,
                "offset": as_f32(votes), "sem_seg_weights": as_f32(loss_w), "center_weights": as_f32(in_center[None]),
                "offset_weights": as_f32(in_offset[None])}
