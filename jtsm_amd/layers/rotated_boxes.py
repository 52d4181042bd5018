"""pairwise_iou_rotated — surface of detectron2/layers/rotated_boxes.py:6-21.  One library call
(csrc/rotated_boxes.hip): the IoU of every pair of (cx, cy, w, h, angle in degrees) boxes, in the arithmetic of the
reference's device code."""
import torch

from .. import _lib as L


@torch.no_grad()
def pairwise_iou_rotated(boxes1: torch.Tensor, boxes2: torch.Tensor) -> torch.Tensor:
    """boxes1 (N,5), boxes2 (M,5) on the device -> IoU (N,M) float32."""
    L.require_gpu(boxes1, boxes2)
    if boxes1.shape[-1] != 5 or boxes2.shape[-1] != 5:
        raise ValueError("pairwise_iou_rotated wants (N,5) and (M,5) boxes, got %s and %s"
                         % (tuple(boxes1.shape), tuple(boxes2.shape)))
    b1 = boxes1.reshape(-1, 5).to(torch.float32).contiguous()
    b2 = boxes2.reshape(-1, 5).to(torch.float32).contiguous()
    n, m = b1.shape[0], b2.shape[0]
    ious = torch.empty((n, m), dtype=torch.float32, device=b1.device)
    L.check(L.lib().jtsm_box_iou_rotated_f32(L.ptr(b1), L.ptr(b2), n, m, L.ptr(ious), L.stream()), "box_iou_rotated")
    return ious
