"""RROIHeads and RotatedFastRCNNOutputLayers — call surface of detectron2/modeling/roi_heads/rotated_fast_rcnn.py:
the standard box head over rotated rois.  Proposals are matched to ground truth through the rotated pairwise IoU,
features are pooled with ROIAlignRotated, the predictor regresses five deltas (Box2BoxTransformRotated) and inference
suppresses duplicates with batched_nms_rotated (csrc/rotated_boxes.hip).  No mask branch."""
from typing import List, Tuple

import torch
import torch.nn.functional as F

from ...layers.nms import batched_nms_rotated
from ...layers.wrappers import cat
from ...structures import Instances, RotatedBoxes, pairwise_iou_rotated
from ..box_regression import Box2BoxTransformRotated
from .fast_rcnn import FastRCNNOutputLayers
from .roi_heads import ROI_HEADS_REGISTRY, StandardROIHeads


@torch.no_grad()
def fast_rcnn_inference_single_image_rotated(boxes, scores, image_shape, score_thresh, nms_thresh, topk_per_image):
    """boxes (R, K*5) or (R, 5), scores (R, K+1) -> (Instances, the kept rows): rows with a non-finite value dropped,
    near-horizontal boxes clipped, scores above the threshold, rotated NMS per class, the topk_per_image best."""
    valid = torch.isfinite(boxes).all(dim=1) & torch.isfinite(scores).all(dim=1)
    if not bool(valid.all()):
        boxes, scores = boxes[valid], scores[valid]
    scores = scores[:, :-1]
    clipped = RotatedBoxes(boxes.reshape(-1, 5).clone())
    clipped.clip(image_shape)
    boxes = clipped.tensor.view(scores.shape[0], -1, 5)
    above = scores > score_thresh
    inds = above.nonzero()
    boxes = boxes[inds[:, 0], 0] if boxes.shape[1] == 1 else boxes[above]
    scores = scores[above]
    keep = batched_nms_rotated(boxes, scores, inds[:, 1], nms_thresh)
    if topk_per_image >= 0:
        keep = keep[:topk_per_image]
    result = Instances(image_shape, pred_boxes=RotatedBoxes(boxes[keep]), scores=scores[keep],
                       pred_classes=inds[keep, 1])
    return result, inds[keep, 0]


def fast_rcnn_inference_rotated(boxes, scores, image_shapes, score_thresh, nms_thresh, topk_per_image):
    per_image = [fast_rcnn_inference_single_image_rotated(b, s, shape, score_thresh, nms_thresh, topk_per_image)
                 for b, s, shape in zip(boxes, scores, image_shapes)]
    return [r for r, _ in per_image], [k for _, k in per_image]


class RotatedFastRCNNOutputLayers(FastRCNNOutputLayers):
    """bbox_pred has reg_classes * 5 outputs; the losses are FastRCNNOutputLayers' over 5-wide deltas."""
    box_dim, transform_type = 5, Box2BoxTransformRotated

    @torch.no_grad()
    def inference(self, predictions: Tuple[torch.Tensor, torch.Tensor], proposals: List[Instances]):
        scores, deltas = predictions
        counts = [len(p) for p in proposals]
        boxes = self.box2box_transform.apply_deltas(deltas, cat([p.proposal_boxes.tensor for p in proposals], dim=0))
        probs = F.softmax(scores, dim=-1)
        return fast_rcnn_inference_rotated(list(boxes.split(counts)), list(probs.split(counts)),
                                           [p.image_size for p in proposals], self.test_score_thresh,
                                           self.test_nms_thresh, self.test_topk_per_image)


@ROI_HEADS_REGISTRY.register()
class RROIHeads(StandardROIHeads):
    pairwise_iou = staticmethod(pairwise_iou_rotated)

    def __init__(self, cfg, input_shape):
        if cfg.MODEL.MASK_ON or cfg.MODEL.get("KEYPOINT_ON", False):
            raise AssertionError("Mask/Keypoints not supported in Rotated ROIHeads.")
        if cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE != "ROIAlignRotated":
            raise AssertionError("RROIHeads pools with ROIAlignRotated, got %s" % cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE)
        super().__init__(cfg, input_shape)

    def _box_predictor(self, cfg, input_shape):
        return RotatedFastRCNNOutputLayers(cfg, input_shape)
