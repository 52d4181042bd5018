"""PCLROIHeads — projects/WSL/wsl/modeling/roi_heads/roi_heads_pcl.py:29-368, box branch only.

_forward_box (:301-368): ROIPool on the box features, every row multiplied by (objectness + 1), the DAN,
WSDDNOutputLayers (MIL loss) and WSL.REFINE_NUM OICROutputLayers branches whose soft-max has the background in column
0.  In training branch k is clustered from the detached scores of branch k - 1 (the MIL scores for k = 0) and trained
with the PCL loss (losses_pcl); inference averages the branches' probabilities and moves the background column behind
the classes (inference(..., pcl_bg=True)).

MI355X mapping: the (objectness + 1) factor is the DAN's per-row `roi_scale` (folded into the plane split in front of
fc1, no multiply pass); cls, det and every branch's cls_score ride in the DAN's node as its tail GEMM.  Clustering and
loss run on the device (layers/pcl.py): between the logits and the loss nothing is read back to the host, where the
reference makes three host round trips per step (pcl.py:26-27, pcl_loss.py:24).  With the backbone frozen (FREEZE_AT
5) the pooled features carry no gradient and no pooling backward runs.  The reference clusters one image per process
(pcl.py:90) and hands branch k + 1 the FIRST image's probabilities (:345-348); here every image is clustered from its
own rows and a branch's loss is the mean over the images."""
from typing import Dict, List, Optional

import torch

from ...layers.shape_spec import ShapeSpec
from ...layers.conv import linear_fused_split
from ...structures import ImageList, Instances
from ..poolers import ROIPooler
from .box_head import build_box_head
from .fast_rcnn_oicr import OICROutputLayers
from .fast_rcnn_wsddn import WSDDNOutputLayers
from .roi_heads import ROI_HEADS_REGISTRY, ROIHeads
from .roi_heads_jtsm import present_things


@ROI_HEADS_REGISTRY.register()
class PCLROIHeads(ROIHeads):
    def __init__(self, cfg, input_shape: Dict[str, ShapeSpec]):
        super().__init__(**ROIHeads.from_config(cfg))
        if cfg.MODEL.MASK_ON or cfg.MODEL.KEYPOINT_ON:
            raise NotImplementedError("PCLROIHeads: only the box branch is implemented (MASK_ON / KEYPOINT_ON)")
        if any(cfg.WSL.REFINE_REG):
            raise NotImplementedError("PCLROIHeads: WSL.REFINE_REG is not implemented — the reference's PCLOutputs "
                                      "cannot compute the regression variant's weights")
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
        self.refine_K = cfg.WSL.REFINE_NUM
        self.box_refinery = []
        for k in range(self.refine_K):
            refinery = OICROutputLayers.from_config(cfg, self.box_head.output_shape.channels, k)
            self.add_module("box_refinery_{}".format(k), refinery)
            self.box_refinery.append(refinery)
        self.train_on_pred_boxes = cfg.MODEL.ROI_BOX_HEAD.TRAIN_ON_PRED_BOXES
        if self.train_on_pred_boxes:
            raise NotImplementedError("PCLROIHeads: TRAIN_ON_PRED_BOXES")
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

    def _predictor_layers(self):
        return [self.box_predictor.cls, self.box_predictor.det] + [r.cls_score for r in self.box_refinery]

    def _logits(self, features, proposals):
        """-> [cls (R, K), det (R, K), branch 0 (R, K+1), ...]: pool, rescale, DAN, every predictor in one GEMM."""
        feats = [features[f] for f in self.box_in_features]
        pooled = self.box_pooler(feats, [x.proposal_boxes for x in proposals])
        scale = torch.cat([x.objectness_logits + 1 for x in proposals], dim=0).to(torch.float32).contiguous()
        mods = self._predictor_layers()
        weights, biases = [m.weight for m in mods], [m.bias for m in mods]
        if getattr(self.box_head, "takes_roi_scale", False):
            out = self.box_head(pooled, roi_scale=scale, tail=(weights, biases))
            if isinstance(out, tuple):                  # (the fused stack: the predictors' GEMM in its node)
                return list(out[1])
            h = out
        else:
            h = self.box_head(pooled * scale.view(-1, 1, 1, 1))
        return list(linear_fused_split(h, weights, biases))

    def _forward_box(self, features, proposals):
        counts = [len(p) for p in proposals]
        outs = self._logits(features, proposals)
        c, d, refine = outs[0], outs[1], outs[2:]
        if self.training:
            offsets = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32).to(c.device,
                                                                                                   non_blocking=True)
            losses, scores, probs = self.box_predictor.score_and_loss(c, d, offsets, self.gt_classes_img_oh,
                                                                      max(max(counts), 1))
            self.pred_class_img_logits = probs
            self.aux = {"mil_scores": scores, "img_probs": probs, "pcl_tables": [], "pcl_probs": []}
            prev = scores                                # (no gradient: a non-differentiable output of the MIL node)
            for k, refinery in enumerate(self.box_refinery):
                losses.update(refinery.losses_pcl((refine[k], None), proposals, prev, self.gt_classes_img_oh,
                                                  offsets=offsets))
                prev = refinery.pcl_probs
                self.aux["pcl_tables"].append(refinery.pcl_tables)
                self.aux["pcl_probs"].append(prev)
            return losses
        zeros = torch.zeros(c.shape[0], self.num_classes * 4, dtype=c.dtype, device=c.device)
        predictions_K = [(z, zeros) for z in refine]
        pred_instances, _, all_scores, all_boxes = self.box_refinery[-1].inference(predictions_K, proposals, pcl_bg=True)
        return pred_instances, all_scores, all_boxes
