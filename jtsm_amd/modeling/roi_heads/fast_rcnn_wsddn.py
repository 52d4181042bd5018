"""WSDDNOutputLayers — the parts of projects/WSL/wsl/modeling/roi_heads/fast_rcnn_wsddn.py:436-850 that ContextLocNet
reaches: two Linear(input -> K) layers `cls`, `det` (:480-503), forward with the ContextLocNet context path
(:560-619: cls(box), det(frame) - det(context)), the MIL BCE loss (:670-692, WSDDNOutputs :346-404, MEAN_LOSS mean or
sum / images), and inference (:727-850: the deltas are zeros, so the boxes are the proposals; per-class NMS).

The MIL scores (softmax over classes x per-image softmax over proposals) and the loss come from the HIP kernels of
layers/wsl_losses.py; NMS and the detections from fast_rcnn_inference (csrc/postprocess.hip)."""
from typing import List

import torch
import torch.nn.functional as F
from torch import nn

from ...layers.cmil import ROIMerge
from ...layers.wrappers import Linear, cat
from ...layers.wsl_losses import mil_loss, mil_scores
from ...structures import Instances
from ..box_regression import Box2BoxTransform
from .fast_rcnn_oicr import fast_rcnn_inference


class WSDDNOutputLayers(nn.Module):
    def __init__(self, input_size, *, num_classes, box2box_transform, test_score_thresh=0.0, test_nms_thresh=0.5,
                 test_topk_per_image=100, mean_loss=True, loss_weight=1.0, cmil=False, display=1280, max_epoch=40,
                 size_epoch=5000):
        super().__init__()
        self.cmil = cmil
        if cmil:
            self.roi_merge = ROIMerge(display, max_epoch, size_epoch)
        self.num_classes = num_classes
        self.box_dim = 4
        self.cls = Linear(input_size, num_classes)
        self.det = Linear(input_size, num_classes)
        nn.init.xavier_uniform_(self.cls.weight)
        nn.init.xavier_uniform_(self.det.weight)
        for l in [self.cls, self.det]:
            nn.init.constant_(l.bias, 0)
        self.box2box_transform = box2box_transform
        self.test_score_thresh = test_score_thresh
        self.test_nms_thresh = test_nms_thresh
        self.test_topk_per_image = test_topk_per_image
        self.mean_loss = mean_loss
        self.loss_weight = {"loss_cls": loss_weight} if isinstance(loss_weight, float) else loss_weight

    @classmethod
    def from_config(cls, cfg, input_size):
        return cls(input_size, num_classes=cfg.MODEL.ROI_HEADS.NUM_CLASSES,
                   box2box_transform=Box2BoxTransform(weights=cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_WEIGHTS),
                   test_score_thresh=cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST,
                   test_nms_thresh=cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST,
                   test_topk_per_image=cfg.TEST.DETECTIONS_PER_IMAGE, mean_loss=cfg.WSL.MEAN_LOSS,
                   cmil=cfg.WSL.CMIL, display=int(1280 / cfg.SOLVER.IMS_PER_BATCH),
                   max_epoch=int(cfg.SOLVER.MAX_ITER / cfg.WSL.SIZE_EPOCH), size_epoch=cfg.WSL.SIZE_EPOCH)

    def logits(self, x, context=False):
        """(C, D): cls(x) and det(x); with context=True x = (box, frame, context) features and D = det(frame) -
        det(context) (forward_contextlocnet, :598-619)."""
        if context:
            x, fx, cx = [t.flatten(1) if t.dim() > 2 else t for t in x]
            return self.cls(x), self.det(fx) - self.det(cx)
        if x.dim() > 2:
            x = torch.flatten(x, start_dim=1)
        return self.cls(x), self.det(x)

    def forward(self, x, proposals: List[Instances] = None, context: bool = False):
        """-> (scores (R, K), proposal_deltas (R, 4K) zeros)."""
        c, d = self.logits(x, context)
        return self.scores_from_logits(c, d, proposals)

    def scores_from_logits(self, c, d, proposals):
        counts = [len(p) for p in proposals] if proposals else [c.shape[0]]
        scores = mil_scores(c, d, counts)
        deltas = torch.zeros(scores.shape[0], self.num_classes * self.box_dim, dtype=scores.dtype, device=scores.device)
        return scores, deltas

    def score_and_loss(self, cls_logits, det_logits, bag_offsets, gt_classes_img_oh, max_bag_rows):
        """The fused form (one forward, one backward launch): -> (losses, scores detached, image probabilities)."""
        loss, scores, probs = mil_loss(cls_logits, det_logits, bag_offsets, gt_classes_img_oh, self.mean_loss,
                                       max_bag_rows)
        return {"loss_cls": loss * self.loss_weight.get("loss_cls", 1.0)}, scores, probs

    def score_and_loss_cmil(self, cls_logits, det_logits, boxes, bag_offsets, gt_classes_img_oh, max_bag_rows):
        """The fused C-MIL form (forward_cmil :621-667 + losses): the un-merged MIL scores (detached), their row sums
        as ROIMerge's ranking, the merge of C and D, and the MIL loss on the merged bags, whose offsets and row counts
        never leave the device.  -> (losses, un-merged scores detached, image probabilities of the merged bags, aux)."""
        with torch.no_grad():
            _, scores, _ = mil_loss(cls_logits.detach(), det_logits.detach(), bag_offsets, gt_classes_img_oh,
                                    self.mean_loss, max_bag_rows)
            row_sums = scores.sum(dim=1)
        lam = self.roi_merge.lam
        MC, MD, I, IC, merged_offsets = self.roi_merge(row_sums, boxes, cls_logits, det_logits, bag_offsets, max_bag_rows)
        loss, _, probs = mil_loss(MC, MD, merged_offsets, gt_classes_img_oh, self.mean_loss, max_bag_rows)
        aux = {"merge_scores": row_sums, "merge_rows": I, "merge_counts": IC, "merged_offsets": merged_offsets,
               "merge_lambda": lam}
        return {"loss_cls": loss * self.loss_weight.get("loss_cls", 1.0)}, scores, probs, aux

    def predict_probs_img(self, predictions, proposals: List[Instances]):
        scores, _ = predictions
        counts = [len(p) for p in proposals] if proposals else [scores.shape[0]]
        img = cat([s.sum(dim=0, keepdim=True) for s in scores.split(counts, dim=0)], dim=0)
        return torch.clamp(img, min=1e-6, max=1.0 - 1e-6)

    def losses(self, predictions, proposals: List[Instances], gt_classes_img_oh):
        """{"loss_cls": BCE of the clamped per-image score sums} — mean, or sum / images (WSDDNOutputs :346-404)."""
        probs = self.predict_probs_img(predictions, proposals)
        target = gt_classes_img_oh.to(probs.dtype)
        if self.mean_loss:
            loss = F.binary_cross_entropy(probs, target, reduction="mean")
        else:
            loss = F.binary_cross_entropy(probs, target, reduction="sum") / target.size(0)
        return {"loss_cls": loss * self.loss_weight.get("loss_cls", 1.0)}

    def predict_probs(self, predictions, proposals: List[Instances]):
        """Per image (R_i, K+1): the scores with a zero background column (:412-422)."""
        scores, _ = predictions
        probs = torch.cat((scores, scores.new_zeros(scores.shape[0], 1)), dim=1)
        return probs.split([len(p) for p in proposals], dim=0)

    def predict_boxes(self, predictions, proposals: List[Instances]):
        """Per image (R_i, 4K): the all-zero deltas applied to the proposals, i.e. the proposals for every class."""
        if not len(proposals):
            return []
        _, deltas = predictions
        boxes = cat([p.proposal_boxes.tensor for p in proposals], dim=0)
        return self.box2box_transform.apply_deltas(deltas, boxes).split([len(p) for p in proposals])

    def inference(self, predictions, proposals: List[Instances]):
        """-> (instances, kept rows, all_scores, all_boxes) per image, as fast_rcnn_inference."""
        boxes = self.predict_boxes(predictions, proposals)
        scores = self.predict_probs(predictions, proposals)
        return fast_rcnn_inference(list(boxes), list(scores), [x.image_size for x in proposals], self.test_score_thresh,
                                   self.test_nms_thresh, self.test_topk_per_image)
