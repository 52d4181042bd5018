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
from typing import Dict, List, Optional

import torch

from ...layers.shape_spec import ShapeSpec
from ...structures import ImageList, Instances
from ..poolers import ROIPooler
from .box_head import build_box_head
from .fast_rcnn_wsddn import WSDDNOutputLayers
from .roi_heads import ROI_HEADS_REGISTRY, ROIHeads
from .roi_heads_jtsm import present_things


@ROI_HEADS_REGISTRY.register()
class ContextLocNetROIHeads(ROIHeads):
    def __init__(self, cfg, input_shape: Dict[str, ShapeSpec]):
        super().__init__(**ROIHeads.from_config(cfg))
        if cfg.MODEL.MASK_ON or cfg.MODEL.KEYPOINT_ON:
            raise NotImplementedError("ContextLocNetROIHeads: only the box branch is implemented (MASK_ON / KEYPOINT_ON)")
        in_features = cfg.MODEL.ROI_HEADS.IN_FEATURES
        self.box_in_features = self.in_features = in_features
        scales = tuple(1.0 / input_shape[k].stride for k in in_features)
        in_channels = [input_shape[f].channels for f in in_features]
        assert len(set(in_channels)) == 1, in_channels
        res = cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION
        pooler_type = cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE
        assert pooler_type == "ROILoopPool", pooler_type
        self.box_pooler = ROIPooler(output_size=res, scales=scales,
                                    sampling_ratio=cfg.MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO, pooler_type=pooler_type)
        self.box_head = build_box_head(cfg, ShapeSpec(channels=in_channels[0], height=res, width=res))
        self.box_predictor = WSDDNOutputLayers.from_config(cfg, self.box_head.output_shape.channels)
        self.aux = {}

    def forward(self, images: ImageList, features: Dict[str, torch.Tensor], proposals: List[Instances],
                targets: Optional[List[Instances]] = None):
        del images
        if self.training:
            assert targets, "'targets' argument is required during training"
            self.gt_classes_img_oh = present_things(targets, self.num_classes)
            return proposals, self._forward_box(features, proposals)
        pred_instances, all_scores, all_boxes = self._forward_box(features, proposals)
        return pred_instances, {}, all_scores, all_boxes

    def forward_with_given_boxes(self, features, instances):
        assert not self.training
        return instances, [], []

    def _logits(self, features, proposals):
        """-> (C (R, K), D (R, K)): pool, rescale, DAN, cls(box) and det(frame) - det(context)."""
        feats = [features[f] for f in self.box_in_features]
        pooled = self.box_pooler(feats, [x.proposal_boxes for x in proposals])
        r = pooled.shape[0] // 3
        scale = torch.cat([x.objectness_logits + 1 for x in proposals], dim=0)
        scale = torch.cat([scale, scale, scale], dim=0).to(torch.float32).contiguous()
        pred = self.box_predictor
        if getattr(self.box_head, "takes_roi_scale", False):
            out = self.box_head(pooled, roi_scale=scale, tail=([pred.cls.weight, pred.det.weight],
                                                               [pred.cls.bias, pred.det.bias]))
            if isinstance(out, tuple):                  # (the fused stack: cls and det over all 3R rows in its node)
                c_all, d_all = out[1]
                self.aux["pooled_rows"] = pooled.shape[0]
                return c_all[:r], d_all[r:2 * r] - d_all[2 * r:]
            h = out
        else:
            h = self.box_head(pooled * scale.view(-1, 1, 1, 1))
        return pred.logits(torch.chunk(h, 3, dim=0), context=True)

    def _forward_box(self, features, proposals):
        counts = [len(p) for p in proposals]
        c, d = self._logits(features, proposals)
        if self.training:
            offsets = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32).to(c.device,
                                                                                                   non_blocking=True)
            losses, scores, probs = self.box_predictor.score_and_loss(c, d, offsets, self.gt_classes_img_oh,
                                                                      max(max(counts), 1))
            self.aux.update(mil_scores=scores, img_probs=probs)
            return losses
        predictions = self.box_predictor.scores_from_logits(c, d, proposals)
        pred_instances, _, all_scores, all_boxes = self.box_predictor.inference(predictions, proposals)
        return pred_instances, all_scores, all_boxes
