"""RRPN — call surface of detectron2/modeling/proposal_generator/rrpn.py:17-203: the RPN over rotated anchors.
Anchors are matched to ground truth through the rotated pairwise IoU, deltas are Box2BoxTransformRotated's five, and
the proposals go through one batched_nms_rotated call per image with the feature level as the class
(csrc/rotated_boxes.hip).  Everything else is the RPN's."""
from typing import List, Tuple

import torch

from ...layers.nms import batched_nms_rotated
from ...structures import Instances, RotatedBoxes, pairwise_iou_rotated
from ..box_regression import Box2BoxTransformRotated
from ..sampling import subsample_labels
from .build import PROPOSAL_GENERATOR_REGISTRY
from .rpn import RPN


@torch.no_grad()
def find_top_rrpn_proposals(proposals: List[torch.Tensor], pred_objectness_logits: List[torch.Tensor],
                            image_sizes: List[Tuple[int, int]], nms_thresh: float, pre_nms_topk: int,
                            post_nms_topk: int, min_box_size: float, training: bool):
    """proposals[l]: (N, H_l*W_l*A, 5), logits[l]: (N, H_l*W_l*A) -> list of N Instances (proposal_boxes,
    objectness_logits) sorted by score: per level the pre_nms_topk best, non-finite rows dropped, near-horizontal
    boxes clipped, empty ones dropped, rotated NMS per level, the post_nms_topk best over all levels."""
    boxes_l, scores_l, level_l = [], [], []
    for level, (boxes, logits) in enumerate(zip(proposals, pred_objectness_logits)):
        k = min(pre_nms_topk, logits.shape[1])
        top, idx = logits.sort(descending=True, dim=1)
        top, idx = top[:, :k], idx[:, :k]
        boxes_l.append(torch.gather(boxes, 1, idx.unsqueeze(2).expand(-1, -1, 5)))
        scores_l.append(top)
        level_l.append(torch.full((k,), level, dtype=torch.int64, device=logits.device))
    all_boxes, all_scores, all_levels = torch.cat(boxes_l, 1), torch.cat(scores_l, 1), torch.cat(level_l)
    out = []
    for n, size in enumerate(image_sizes):
        boxes, scores, levels = RotatedBoxes(all_boxes[n].clone()), all_scores[n], all_levels
        finite = torch.isfinite(boxes.tensor).all(dim=1) & torch.isfinite(scores)
        if not bool(finite.all()):
            if training:
                raise FloatingPointError("Predicted boxes or scores contain Inf/NaN. Training has diverged.")
            boxes, scores, levels = boxes[finite], scores[finite], levels[finite]
        boxes.clip(size)
        keep = boxes.nonempty(threshold=min_box_size)
        if int(keep.sum()) != len(boxes):
            boxes, scores, levels = boxes[keep], scores[keep], levels[keep]
        keep = batched_nms_rotated(boxes.tensor, scores, levels, nms_thresh)[:post_nms_topk]
        out.append(Instances(size, proposal_boxes=boxes[keep], objectness_logits=scores[keep]))
    return out


@PROPOSAL_GENERATOR_REGISTRY.register()
class RRPN(RPN):
    def __init__(self, cfg, input_shape):
        super().__init__(cfg, input_shape)
        if self.anchor_generator.box_dim != 5:
            raise ValueError("RRPN wants 5-wide anchors (MODEL.ANCHOR_GENERATOR.NAME = RotatedAnchorGenerator)")
        self.box2box_transform = Box2BoxTransformRotated(weights=cfg.MODEL.RPN.BBOX_REG_WEIGHTS)
        if self.anchor_boundary_thresh >= 0:
            raise NotImplementedError("anchor_boundary_thresh is a legacy option not implemented for RRPN.")

    def match_anchors(self, anchors: List[RotatedBoxes], gt_instances: List[Instances]):
        """Per image, before sub-sampling: the matched ground-truth index and the label (-1 / 0 / 1) of every anchor."""
        anchors = RotatedBoxes.cat(anchors)
        return [self.anchor_matcher(pairwise_iou_rotated(inst.gt_boxes, anchors)) for inst in gt_instances]

    @torch.no_grad()
    def label_and_sample_anchors(self, anchors: List[RotatedBoxes], gt_instances: List[Instances]):
        flat = RotatedBoxes.cat(anchors)
        labels, matched = [], []
        for inst, (idx, lab) in zip(gt_instances, self.match_anchors(anchors, gt_instances)):
            gt = inst.gt_boxes
            lab = lab.to(device=gt.tensor.device)
            pos, neg = subsample_labels(lab, self.batch_size_per_image, self.positive_fraction, 0)
            sampled = torch.full_like(lab, -1)
            sampled[pos] = 1
            sampled[neg] = 0
            labels.append(sampled)
            matched.append(gt.tensor[idx] if len(gt) else torch.zeros_like(flat.tensor))
        return labels, matched

    @torch.no_grad()
    def predict_proposals(self, anchors, logits, deltas, image_sizes):
        decoded = []
        for a, d in zip(anchors, deltas):
            n = d.shape[0]
            flat = a.tensor.unsqueeze(0).expand(n, -1, -1).reshape(-1, 5)
            decoded.append(self.box2box_transform.apply_deltas(d.detach().reshape(-1, 5), flat).view(n, -1, 5))
        return find_top_rrpn_proposals(decoded, [z.detach() for z in logits], image_sizes, self.nms_thresh,
                                       self.pre_nms_topk[self.training], self.post_nms_topk[self.training],
                                       self.min_box_size, self.training)
