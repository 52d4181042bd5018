"""RotatedBoxes — detectron2/structures/rotated_boxes.py:14-481: a thin wrapper of an (N, 5) float32 tensor of
(x_center, y_center, width, height, angle in degrees, counter-clockwise positive), and pairwise_iou over the device
kernel of layers/rotated_boxes.py.  Method names are the reference's; the bodies are this repo's."""
import math

import torch

from ..layers.rotated_boxes import pairwise_iou_rotated


class RotatedBoxes(object):
    __slots__ = ("tensor",)

    def __init__(self, tensor):
        t = tensor if isinstance(tensor, torch.Tensor) else torch.as_tensor(tensor, dtype=torch.float32)
        t = t.to(torch.float32)
        if t.numel() == 0:
            t = t.new_zeros((0, 5))
        if t.dim() != 2 or t.shape[1] != 5:
            raise ValueError("RotatedBoxes wants an (N, 5) tensor, got %s" % (tuple(t.shape),))
        self.tensor = t

    def __len__(self):
        return self.tensor.shape[0]

    def __iter__(self):
        return iter(self.tensor)

    def __getitem__(self, index):
        rows = self.tensor[index]
        if rows.dim() == 1:
            rows = rows.unsqueeze(0)
        return RotatedBoxes(rows)

    def __repr__(self):
        return "RotatedBoxes(%s)" % (self.tensor,)

    @property
    def device(self):
        return self.tensor.device

    def to(self, *args, **kwargs):
        return RotatedBoxes(self.tensor.to(*args, **kwargs))

    def clone(self):
        return RotatedBoxes(self.tensor.clone())

    @classmethod
    def cat(cls, boxes_list):
        rows = [b.tensor for b in boxes_list]
        return cls(torch.cat(rows, dim=0) if rows else torch.empty(0))

    def area(self):
        """width x height: what assigns a rotated box its FPN level (rotated_boxes.py:238-246)."""
        return self.tensor[:, 2] * self.tensor[:, 3]

    def get_centers(self):
        return self.tensor[:, :2]

    def normalize_angles(self):
        """In place: angles to [-180, 180) (rotated_boxes.py:246-250)."""
        self.tensor[:, 4] = (self.tensor[:, 4] + 180.0) % 360.0 - 180.0

    def clip(self, box_size, clip_angle_threshold=1.0):
        """In place (rotated_boxes.py:252-300): normalise the angles, then clip the boxes that are horizontal within
        clip_angle_threshold degrees to [0, width] x [0, height] as xyxy boxes; the others are left alone (there is
        no one way to clip a turned box, and ROIAlignRotated copes with boxes that leave the image)."""
        h, w = box_size
        self.normalize_angles()
        t = self.tensor
        idx = torch.where(torch.abs(t[:, 4]) <= clip_angle_threshold)[0]
        x1 = (t[idx, 0] - t[idx, 2] / 2.0).clamp_(min=0, max=w)
        y1 = (t[idx, 1] - t[idx, 3] / 2.0).clamp_(min=0, max=h)
        x2 = (t[idx, 0] + t[idx, 2] / 2.0).clamp_(min=0, max=w)
        y2 = (t[idx, 1] + t[idx, 3] / 2.0).clamp_(min=0, max=h)
        t[idx, 0] = (x1 + x2) / 2.0
        t[idx, 1] = (y1 + y2) / 2.0
        t[idx, 2] = torch.min(t[idx, 2], x2 - x1)     # rounding must not grow a side
        t[idx, 3] = torch.min(t[idx, 3], y2 - y1)

    def nonempty(self, threshold=0.0):
        return (self.tensor[:, 2] > threshold) & (self.tensor[:, 3] > threshold)

    def inside_box(self, box_size, boundary_threshold=0):
        """Whether the horizontal bounding rectangle of each box lies within [0, width] x [0, height], give or take
        boundary_threshold (rotated_boxes.py:346-381)."""
        height, width = box_size
        cx, cy = self.tensor[..., 0], self.tensor[..., 1]
        half_w, half_h = self.tensor[..., 2] / 2.0, self.tensor[..., 3] / 2.0
        a = self.tensor[..., 4]
        c, s = torch.abs(torch.cos(a * math.pi / 180.0)), torch.abs(torch.sin(a * math.pi / 180.0))
        dx, dy = c * half_w + s * half_h, c * half_h + s * half_w
        return ((cx - dx >= -boundary_threshold) & (cy - dy >= -boundary_threshold)
                & (cx + dx < width + boundary_threshold) & (cy + dy < height + boundary_threshold))

    def scale(self, scale_x, scale_y):
        """In place (rotated_boxes.py:390-453).  scale_x == scale_y scales centre and sides and leaves the angle; an
        anisotropic resize turns the rectangle into a parallelogram, which is replaced by the rectangle through the
        images of the mid-points of its left and top edges: w *= |(sx c, sy s)|, h *= |(sx s, sy c)|, angle =
        atan2(sx s, sy c)."""
        if scale_x == scale_y:
            self.tensor[:, :4] *= scale_x
            return
        t = self.tensor
        theta = t[:, 4] * math.pi / 180.0
        c, s = torch.cos(theta), torch.sin(theta)
        t[:, 0] *= scale_x
        t[:, 1] *= scale_y
        t[:, 2] *= torch.sqrt((scale_x * c) ** 2 + (scale_y * s) ** 2)
        t[:, 3] *= torch.sqrt((scale_x * s) ** 2 + (scale_y * c) ** 2)
        t[:, 4] = torch.atan2(scale_x * s, scale_y * c) * 180 / math.pi


def pairwise_iou(boxes1, boxes2):
    """IoU (N, M) of two RotatedBoxes on the device (rotated_boxes.py:466-481)."""
    return pairwise_iou_rotated(boxes1.tensor, boxes2.tensor)
