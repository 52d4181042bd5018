"""ContextLocNetROIHeads — projects/WSL/wsl/modeling/roi_heads/roi_heads_contextlocnet.py:28-335, box branch only.

_forward_box (:277-335): ROILoopPool on the box features gives 3R rows (box, frame, context blocks), all of them are
multiplied by (objectness + 1), the DAN runs on the 3R rows, and the result splits into three chunks that
WSDDNOutputLayers reads with context=True (cls(box), det(frame) - det(context)).

MI355X mapping: the (objectness + 1) factor, tiled x3, is the DAN's per-row `roi_scale` — folded into the plane split in
front of fc1 and into fc1's data-gradient epilogue, no multiply pass (one multiply, as the reference: the same bits).
cls and det ride in the DAN's node as its tail GEMM over all 3R rows; the rows each block needs are sliced from it.
With the backbone frozen (FREEZE_AT 5) the pooled features carry no gradient: the stack then computes no data
gradient for fc1 and no pooling backward runs.  Training keeps every proposal (the WSL label_and_sample_proposals
keeps all of them, roi_heads.py:253-254, and nothing here reads a per-proposal label)."""
from typing import Dict

import torch

from ...layers.shape_spec import ShapeSpec
from .roi_heads import ROI_HEADS_REGISTRY, bag_offsets
from .roi_heads_wsl import WSLBoxHeads


@ROI_HEADS_REGISTRY.register()
class ContextLocNetROIHeads(WSLBoxHeads):
    def __init__(self, cfg, input_shape: Dict[str, ShapeSpec]):
        assert cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE == "ROILoopPool", cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE
        super().__init__(cfg, input_shape)

    def _logits(self, features, proposals):
        """-> (C (R, K), D (R, K)): pool, rescale, DAN, cls(box) and det(frame) - det(context)."""
        pred = self.box_predictor
        h, outs = self._pooled_hidden(features, proposals, [pred.cls, pred.det], blocks=3)
        if outs is None:
            return pred.logits(torch.chunk(h, 3, dim=0), context=True)
        c_all, d_all = outs                             # (cls and det over all 3R rows)
        r = c_all.shape[0] // 3
        self.aux["pooled_rows"] = c_all.shape[0]
        return c_all[:r], d_all[r:2 * r] - d_all[2 * r:]

    def _forward_box(self, features, proposals):
        counts = [len(p) for p in proposals]
        c, d = self._logits(features, proposals)
        if self.training:
            losses, scores, probs = self.box_predictor.score_and_loss(c, d, bag_offsets(counts, c.device),
                                                                      self.gt_classes_img_oh, max(max(counts), 1))
            self.aux.update(mil_scores=scores, img_probs=probs)
            return losses
        predictions = self.box_predictor.scores_from_logits(c, d, proposals)
        pred_instances, _, all_scores, all_boxes = self.box_predictor.inference(predictions, proposals)
        return pred_instances, all_scores, all_boxes
