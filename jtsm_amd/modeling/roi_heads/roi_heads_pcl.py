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
from typing import Dict

import torch

from ...layers.conv import linear_fused_split
from ...layers.shape_spec import ShapeSpec
from .roi_heads import ROI_HEADS_REGISTRY, bag_offsets
from .roi_heads_wsl import WSLBoxHeads


@ROI_HEADS_REGISTRY.register()
class PCLROIHeads(WSLBoxHeads):
    def __init__(self, cfg, input_shape: Dict[str, ShapeSpec]):
        if any(cfg.WSL.REFINE_REG):
            raise NotImplementedError("PCLROIHeads: WSL.REFINE_REG is not implemented — the reference's PCLOutputs "
                                      "cannot compute the regression variant's weights")
        super().__init__(cfg, input_shape)
        self._build_refinery(cfg)
        self.train_on_pred_boxes = cfg.MODEL.ROI_BOX_HEAD.TRAIN_ON_PRED_BOXES
        if self.train_on_pred_boxes:
            raise NotImplementedError("PCLROIHeads: TRAIN_ON_PRED_BOXES")

    def _predictor_layers(self):
        return [self.box_predictor.cls, self.box_predictor.det] + [r.cls_score for r in self.box_refinery]

    def _logits(self, features, proposals):
        """-> [cls (R, K), det (R, K), branch 0 (R, K+1), ...]: pool, rescale, DAN, every predictor in one GEMM."""
        mods = self._predictor_layers()
        h, outs = self._pooled_hidden(features, proposals, mods)
        return outs or list(linear_fused_split(h, [m.weight for m in mods], [m.bias for m in mods]))

    def _forward_box(self, features, proposals):
        counts = [len(p) for p in proposals]
        outs = self._logits(features, proposals)
        c, d, refine = outs[0], outs[1], outs[2:]
        if self.training:
            offsets = bag_offsets(counts, c.device)
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
