"""WSLBoxHeads — what the box-branch-only WSL heads (ContextLocNetROIHeads, PCLROIHeads, OICRROIHeads) share: the pooler,
the DAN and WSDDNOutputLayers, the optional OICROutputLayers refinery, forward, and the pool -> (objectness + 1) ->
DAN -> predictor-GEMM step.  Each head keeps its own _forward_box, refusals and predictor list."""
from typing import Dict, List, Optional

import torch

from ...layers.shape_spec import ShapeSpec
from ...structures import ImageList, Instances
from ..poolers import ROIPooler
from .box_head import build_box_head
from .fast_rcnn_oicr import OICROutputLayers
from .fast_rcnn_wsddn import WSDDNOutputLayers
from .roi_heads import ROIHeads
from .roi_heads_jtsm import present_things


class WSLBoxHeads(ROIHeads):
    def __init__(self, cfg, input_shape: Dict[str, ShapeSpec]):
        super().__init__(**ROIHeads.from_config(cfg))
        if cfg.MODEL.MASK_ON or cfg.MODEL.KEYPOINT_ON:
            raise NotImplementedError("%s: only the box branch is implemented (MASK_ON / KEYPOINT_ON)"
                                      % type(self).__name__)
        in_features = cfg.MODEL.ROI_HEADS.IN_FEATURES
        self.box_in_features = self.in_features = in_features
        scales = tuple(1.0 / input_shape[k].stride for k in in_features)
        in_channels = [input_shape[f].channels for f in in_features]
        assert len(set(in_channels)) == 1, in_channels
        res = cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION
        self.box_pooler = ROIPooler(output_size=res, scales=scales,
                                    sampling_ratio=cfg.MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO,
                                    pooler_type=cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE)
        self.box_head = build_box_head(cfg, ShapeSpec(channels=in_channels[0], height=res, width=res))
        self.box_predictor = WSDDNOutputLayers.from_config(cfg, self.box_head.output_shape.channels)
        self.aux = {}

    def _build_refinery(self, cfg):
        """box_refinery / box_refinery_{k}: WSL.REFINE_NUM OICROutputLayers, registered in k order."""
        self.refine_K = cfg.WSL.REFINE_NUM
        self.box_refinery = []
        for k in range(self.refine_K):
            refinery = OICROutputLayers.from_config(cfg, self.box_head.output_shape.channels, k)
            self.add_module("box_refinery_{}".format(k), refinery)
            self.box_refinery.append(refinery)

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

    def _pooled_hidden(self, features, proposals, layers, blocks=1):
        """-> (h, outs): pool, rescale every row by (objectness + 1) (tiled over the pooler's `blocks` row blocks), DAN.
        `outs` is the list the predictor `layers` give as the DAN's tail GEMM over all rows, or None where the box
        head did not run it: the caller then applies the predictors to h."""
        feats = [features[f] for f in self.box_in_features]
        pooled = self.box_pooler(feats, [x.proposal_boxes for x in proposals])
        scale = torch.cat([x.objectness_logits + 1 for x in proposals] * blocks, dim=0).to(torch.float32).contiguous()
        if getattr(self.box_head, "takes_roi_scale", False):
            out = self.box_head(pooled, roi_scale=scale, tail=([m.weight for m in layers], [m.bias for m in layers]))
            if isinstance(out, tuple):                  # (the fused stack: the predictors' GEMM in its node)
                return out[0], list(out[1])
            return out, None
        return self.box_head(pooled * scale.view(-1, 1, 1, 1)), None
