"""CMILROIHeads — projects/WSL/wsl/modeling/roi_heads/roi_heads_cmil.py:33-479, box branch only.

_forward_box (:351-479): the pooler (ROILoopPool in the shipped configuration: 3R rows, cls(box) and det(frame) -
det(context) as ContextLocNet; any other pooler: plain cls / det), every row multiplied by (objectness + 1), the DAN,
WSDDNOutputLayers with cmil=True — the continuation merge of C and D in front of the MIL loss — and WSL.REFINE_NUM
OICROutputLayers branches.  In training branch k mines the top-scoring proposal of every present class from the detached
predictions of branch k - 1 (get_pgt_top_k, top 1), matches the proposals to it for the regression targets
(label_and_sample_proposals), and takes its classes and loss weights from ROILabel(0.6, 0.4, 0.1, 32, 96, 1) (:193,
:419-442).  Inference averages the branches (:466-478).

The declared reading: as shipped the reference's C-MIL training step cannot run — forward returns four
values where losses unpacks two, predictions[0] has merged rows where the mining indexes proposals, and J is square
for one image per GPU only.  Taken here is its evident intent: the MIL loss on the merged rows, the image
probabilities from them, branch 0 mined and labelled from the un-merged scores, merge and labelling per image.

MI355X mapping: as OICROIHeads — every predictor rides in the DAN's tail GEMM (over the 3R rows with ROILoopPool; the
box block's rows are sliced from it), and a step reads nothing back: ROIMerge leaves the merged bags' offsets on the
device for `mil_loss`, ROILabel draws its visiting order with torch.randperm on the device."""
from typing import Dict

import torch

from ...layers.cmil import ROILabel
from ...layers.conv import linear_fused_split
from ...layers.mining import match_label, mine_top1, row_lse
from ...layers.shape_spec import ShapeSpec
from .roi_heads import ROI_HEADS_REGISTRY, bag_offsets
from .roi_heads_jtsm import class_lists
from .roi_heads_wsl import WSLBoxHeads


@ROI_HEADS_REGISTRY.register()
class CMILROIHeads(WSLBoxHeads):
    def __init__(self, cfg, input_shape: Dict[str, ShapeSpec]):
        if cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG:
            raise NotImplementedError("CMILROIHeads: CLS_AGNOSTIC_BBOX_REG")
        if cfg.MODEL.ROI_BOX_HEAD.TRAIN_ON_PRED_BOXES:
            raise NotImplementedError("CMILROIHeads: TRAIN_ON_PRED_BOXES")
        if cfg.WSL.SAMPLING.SAMPLING_ON:
            raise NotImplementedError("CMILROIHeads: WSL.SAMPLING (label_and_sample_proposals_wsl)")
        super().__init__(cfg, input_shape)
        assert len(cfg.WSL.REFINE_REG) >= cfg.WSL.REFINE_NUM, "WSL.REFINE_REG needs one entry per refinement branch"
        self._build_refinery(cfg)
        self.blocks = 3 if cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE == "ROILoopPool" else 1
        self.roi_label = ROILabel(0.6, 0.4, 0.1, 32, 96, 1)       # (:193)
        self.label_generator = None                               # optional torch.Generator of ROILabel's draws

    def _predictor_layers(self):
        mods = [self.box_predictor.cls, self.box_predictor.det]
        for r in self.box_refinery:
            mods += [r.cls_score] + ([r.bbox_pred] if r.has_reg else [])
        return mods

    def _logits(self, features, proposals):
        """-> [C (R, K), D (R, K), branch 0 logits (R, K+1), (branch 0 deltas (R, 4K),) ...].  With ROILoopPool the
        predictors run over the 3R rows: D = det(frame) - det(context), everything else reads the box block."""
        mods = self._predictor_layers()
        h, outs = self._pooled_hidden(features, proposals, mods, blocks=self.blocks)
        if outs is None:
            outs = list(linear_fused_split(h, [m.weight for m in mods], [m.bias for m in mods]))
        if self.blocks == 1:
            return outs
        r = outs[0].shape[0] // 3
        self.aux["pooled_rows"] = outs[0].shape[0]
        return [outs[0][:r], outs[1][r:2 * r] - outs[1][2 * r:]] + [o[:r] for o in outs[2:]]

    def _branch_outputs(self, outs):
        """[(logits, deltas or None)] of the refinement branches from the predictor GEMM's column slices."""
        col, pairs = 2, []
        for r in self.box_refinery:
            pairs.append((outs[col], outs[col + 1] if r.has_reg else None))
            col += 2 if r.has_reg else 1
        return pairs

    def _forward_box(self, features, proposals):
        counts = [len(p) for p in proposals]
        self.aux = {}
        outs = self._logits(features, proposals)
        c, d, refine = outs[0], outs[1], self._branch_outputs(outs)
        if not self.training:
            zeros = None
            predictions_K = []
            for z, dl in refine:
                if dl is None:      # a branch without regression hands in zero deltas (OICROutputLayers.forward)
                    if zeros is None:
                        zeros = torch.zeros(z.shape[0], self.num_classes * 4, dtype=z.dtype, device=z.device)
                    dl = zeros
                predictions_K.append((z, dl))
            pred_instances, _, all_scores, all_boxes = self.box_refinery[-1].inference(predictions_K, proposals)
            return pred_instances, all_scores, all_boxes

        dev = c.device
        offsets = bag_offsets(counts, dev)
        all_boxes = torch.cat([p.proposal_boxes.tensor for p in proposals]).contiguous()
        losses, scores, img_probs, merge_aux = self.box_predictor.score_and_loss_cmil(
            c, d, all_boxes, offsets, self.gt_classes_img_oh, max(max(counts), 1))
        self.pred_class_img_logits = img_probs
        cls, cnt = class_lists(self.gt_classes_img_oh)
        self.aux.update(mil_scores=scores, img_probs=img_probs, things_cnt=cnt, **merge_aux)

        # branch k is labelled from branch k - 1's detached predictions (k = 0: the un-merged MIL scores, the proposals)
        prev_logits = prev_deltas = None
        for k, (refinery, (z, dl)) in enumerate(zip(self.box_refinery, refine)):
            lse = row_lse(prev_logits) if k else None
            src = prev_logits if k else scores
            pg = mine_top1(src, all_boxes, offsets, cls, cnt, img_probs, lse=lse, deltas=prev_deltas)
            lab = match_label(all_boxes, offsets, pg, cls, cnt, self.num_classes)
            rl = self.roi_label(src, all_boxes, offsets, cls, cnt, img_probs, rows_per_image=counts,
                                generator=self.label_generator, lse=lse, num_classes=self.num_classes)
            self.aux["pgt_rows_r%d" % k], self.aux["labels_r%d" % k] = pg["idx"], rl["labels"]
            self.aux["weights_r%d" % k], self.aux["perm_r%d" % k] = rl["weights"], rl["perm"]
            self.aux["seed_rows_r%d" % k], self.aux["seed_num_r%d" % k] = rl["seed_rows"], rl["seed_num"]
            self.aux["logits_r%d" % k], self.aux["deltas_r%d" % k] = z.detach(), (dl.detach() if dl is not None else None)
            losses.update(refinery.losses((z, dl), all_boxes, rl["labels"], lab["boxes"], rl["weights"]))
            prev_logits, prev_deltas = self.aux["logits_r%d" % k], self.aux["deltas_r%d" % k]
        return losses
