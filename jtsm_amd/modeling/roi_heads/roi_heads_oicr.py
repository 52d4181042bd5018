"""OICRROIHeads — projects/WSL/wsl/modeling/roi_heads/roi_heads_oicr.py:33-811, box branch only.

_forward_box (:373-478): ROIPool on the box features, every row multiplied by (objectness + 1), the DAN,
WSDDNOutputLayers (MIL loss) and WSL.REFINE_NUM OICROutputLayers branches.  In training branch k is labelled from the
detached predictions of branch k - 1 (the MIL scores and the raw proposals for k = 0): pseudo ground truth is the
top-scoring proposal of every present class (get_pgt_top_k, :660-811) or, with WSL.REFINE_MIST, the top 15 % of every
present class after one class-agnostic NMS at IoU 0.2 (get_pgt_mist, :550-591; branch 0's losses then count three
times, :423-424); every proposal takes the class of the pseudo box it overlaps best (IoU >= 0.5, no sub-sampling,
label_and_sample_proposals) and the branch trains with the weighted cross-entropy and the weighted smooth-L1 loss.
Inference averages the branches' probabilities and deltas (:470-478).

MI355X mapping: as PCLROIHeads — the (objectness + 1) factor is the DAN's per-row `roi_scale`, cls, det and every
branch's cls_score / bbox_pred ride in the DAN's node as its tail GEMM.  A refinement round is three library calls —
mining (layers/mining.py mine_top1, or layers/mist.py mine_top_p), labelling (match_label, which takes the padded
survivor list with its device-side count) and the fused loss — and reads nothing back to the host, MIST included,
where the reference's topk / batched_nms / indexing chain brings the list lengths to the host in every round."""
from typing import Dict

import torch

from ...layers.conv import linear_fused_split
from ...layers.mining import match_label, mine_top1, row_lse
from ...layers.mist import mine_top_p, top_p_counts
from ...layers.shape_spec import ShapeSpec
from .roi_heads import ROI_HEADS_REGISTRY, bag_offsets
from .roi_heads_jtsm import class_lists
from .roi_heads_wsl import WSLBoxHeads

MIST_TOP_PRO = 0.15        # get_pgt_mist's top_pro default (:550)
MIST_NMS_THRESH = 0.2      # (:566)
MIST_FIRST_BRANCH_WEIGHT = 3


@ROI_HEADS_REGISTRY.register()
class OICRROIHeads(WSLBoxHeads):
    def __init__(self, cfg, input_shape: Dict[str, ShapeSpec]):
        if cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG:
            raise NotImplementedError("OICRROIHeads: CLS_AGNOSTIC_BBOX_REG")
        if cfg.MODEL.ROI_BOX_HEAD.TRAIN_ON_PRED_BOXES:
            raise NotImplementedError("OICRROIHeads: TRAIN_ON_PRED_BOXES")
        if cfg.WSL.SAMPLING.SAMPLING_ON:
            raise NotImplementedError("OICRROIHeads: WSL.SAMPLING (label_and_sample_proposals_wsl)")
        super().__init__(cfg, input_shape)
        self.refine_mist = cfg.WSL.REFINE_MIST
        assert len(cfg.WSL.REFINE_REG) >= cfg.WSL.REFINE_NUM, "WSL.REFINE_REG needs one entry per refinement branch"
        self._build_refinery(cfg)

    def _predictor_layers(self):
        mods = [self.box_predictor.cls, self.box_predictor.det]
        for r in self.box_refinery:
            mods += [r.cls_score] + ([r.bbox_pred] if r.has_reg else [])
        return mods

    def _logits(self, features, proposals):
        """-> [cls (R, K), det (R, K), branch 0 logits (R, K+1), (branch 0 deltas (R, 4K),) ...]: pool, rescale, DAN,
        every predictor in one GEMM."""
        mods = self._predictor_layers()
        h, outs = self._pooled_hidden(features, proposals, mods)
        return outs or list(linear_fused_split(h, [m.weight for m in mods], [m.bias for m in mods]))

    def _branch_outputs(self, outs):
        """[(logits, deltas or None)] of the refinement branches from the predictor GEMM's column slices."""
        col, pairs = 2, []
        for r in self.box_refinery:
            pairs.append((outs[col], outs[col + 1] if r.has_reg else None))
            col += 2 if r.has_reg else 1
        return pairs

    def _forward_box(self, features, proposals):
        counts = [len(p) for p in proposals]
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
        losses, scores, img_probs = self.box_predictor.score_and_loss(c, d, offsets, self.gt_classes_img_oh,
                                                                      max(max(counts), 1))
        self.pred_class_img_logits = img_probs
        all_boxes = torch.cat([p.proposal_boxes.tensor for p in proposals]).contiguous()
        cls, cnt = class_lists(self.gt_classes_img_oh)
        self.aux = {"mil_scores": scores, "img_probs": img_probs, "things_cnt": cnt}
        if self.refine_mist:
            top_t, t_max = top_p_counts(counts, MIST_TOP_PRO, dev)

        # branch k is labelled from branch k - 1's detached predictions (k = 0: the MIL scores, the raw proposals)
        prev_logits = prev_deltas = None
        for k, (refinery, (z, dl)) in enumerate(zip(self.box_refinery, refine)):
            lse = row_lse(prev_logits) if k else None
            src = prev_logits if k else scores
            if self.refine_mist:
                pg = mine_top_p(src, all_boxes, offsets, cls, cnt, top_t, t_max, lse=lse, deltas=prev_deltas,
                                iou_thresh=MIST_NMS_THRESH)
                lab = match_label(all_boxes, offsets, pg, pg["classes"], pg["num"], self.num_classes)
                self.aux["pgt_rows_r%d" % k], self.aux["pgt_num_r%d" % k] = pg["rows"], pg["num"]
                self.aux["pgt_classes_r%d" % k] = pg["classes"]
            else:
                pg = mine_top1(src, all_boxes, offsets, cls, cnt, img_probs, lse=lse, deltas=prev_deltas)
                lab = match_label(all_boxes, offsets, pg, cls, cnt, self.num_classes)
                self.aux["pgt_rows_r%d" % k], self.aux["pgt_num_r%d" % k] = pg["idx"], cnt
            self.aux["labels_r%d" % k] = lab["labels"]
            self.aux["logits_r%d" % k], self.aux["deltas_r%d" % k] = z.detach(), (dl.detach() if dl is not None else None)
            losses_k = refinery.losses((z, dl), all_boxes, lab["labels"], lab["boxes"], lab["weights"])
            if self.refine_mist and k == 0:
                losses_k = {n: v * MIST_FIRST_BRANCH_WEIGHT for n, v in losses_k.items()}
            losses.update(losses_k)
            prev_logits, prev_deltas = self.aux["logits_r%d" % k], self.aux["deltas_r%d" % k]
        return losses
