"""ROI heads base — the parts of projects/WSL/wsl/modeling/roi_heads/roi_heads.py on the JTSM path:
registry + build_roi_heads (:25-43), get_image_level_gt (:145-161), select_foreground_proposals,
ROIHeads.label_and_sample_proposals (:222-370; the WSL variant keeps EVERY proposal, :253-254)."""
from typing import List

import torch

from ...structures import Boxes, Instances, pairwise_iou
from ...utils.registry import Registry
from ..matcher import Matcher

ROI_HEADS_REGISTRY = Registry("ROI_HEADS")


def build_roi_heads(cfg, input_shape):
    return ROI_HEADS_REGISTRY.get(cfg.MODEL.ROI_HEADS.NAME)(cfg, input_shape)


def select_foreground_proposals(proposals: List[Instances], bg_label: int):
    fg_proposals, fg_selection_masks = [], []
    for proposals_per_image in proposals:
        gt_classes = proposals_per_image.gt_classes
        fg_selection_mask = (gt_classes != -1) & (gt_classes != bg_label)
        fg_idxs = fg_selection_mask.nonzero().squeeze(1)
        fg_proposals.append(proposals_per_image[fg_idxs])
        fg_selection_masks.append(fg_selection_mask)
    return fg_proposals, fg_selection_masks


def select_proposals_with_visible_keypoints(proposals: List[Instances]):
    """detectron2/modeling/roi_heads/roi_heads.py:77-121: keep the proposals whose matched instance has at least one
    labelled keypoint (v >= 1) inside the proposal box, edges included; the others would add nothing to the loss."""
    ret = []
    for proposals_per_image in proposals:
        if len(proposals_per_image) == 0 or not proposals_per_image.has("gt_keypoints"):
            ret.append(proposals_per_image)
            continue
        gt_keypoints = proposals_per_image.gt_keypoints.tensor
        vis_mask = gt_keypoints[:, :, 2] >= 1
        xs, ys = gt_keypoints[:, :, 0], gt_keypoints[:, :, 1]
        box = proposals_per_image.proposal_boxes.tensor.unsqueeze(dim=1)     # (#proposals, 1, 4)
        kp_in_box = (xs >= box[:, :, 0]) & (xs <= box[:, :, 2]) & (ys >= box[:, :, 1]) & (ys <= box[:, :, 3])
        selection = (kp_in_box & vis_mask).any(dim=1)
        ret.append(proposals_per_image[selection.nonzero().squeeze(1)])
    return ret


@torch.no_grad()
def get_image_level_gt(targets, num_classes):
    """Per image: sorted unique thing classes (float/int64 copies) and their one-hot (B,num_classes)."""
    if targets is None:
        return None, None, None
    gt_classes_img = [torch.unique(t.gt_classes, sorted=True) for t in targets]
    gt_classes_img_int = [gt.to(torch.int64) for gt in gt_classes_img]
    oh = torch.zeros((len(targets), num_classes), dtype=torch.float, device=gt_classes_img[0].device)
    for i, gt in enumerate(gt_classes_img_int):
        oh[i, gt] = 1
    return gt_classes_img, gt_classes_img_int, oh


def bag_offsets(counts, device):
    """int32 (B+1,) device tensor of the images' first rows in the concatenated proposal list."""
    return torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32).to(device, non_blocking=True)


def cropped_mask_targets(fg, targets, side):
    """Per foreground roi its matched instance's bitmask cropped to the roi at side x side (crop_and_resize =
    ROIAlign(1.0, sampling 0, aligned) >= 0.5): (R, side, side) bool, concatenated over the images."""
    from ...layers.roi_align import roi_align

    tgt = []
    for p, t in zip(fg, targets):
        if len(p) == 0:
            continue
        if not isinstance(t.gt_masks, torch.Tensor) or t.gt_masks.dim() != 3:
            # (the reference's default INPUT.MASK_FORMAT is "polygon": PolygonMasks rasterised per roi by
            # pycocotools — outside the HIP scope; BitMasks users pass `.tensor`)
            raise TypeError("StandardROIHeads mask branch: gt_masks must be a (G, H, W) bitmask tensor "
                            "(INPUT.MASK_FORMAT = 'bitmask'), got %r" % type(t.gt_masks).__name__)
        masks = t.gt_masks.to(torch.float32)[:, None]                         # (G, 1, H, W) bitmasks
        rois = torch.cat([p.matched_gt_idx.to(torch.float32)[:, None], p.proposal_boxes.tensor], dim=1)
        tgt.append(roi_align(masks, rois, (side, side), 1.0, 0, True)[:, 0] >= 0.5)
    return torch.cat(tgt) if tgt else None


class ROIHeads(torch.nn.Module):
    def __init__(self, *, num_classes, batch_size_per_image, positive_fraction, proposal_matcher,
                 proposal_append_gt=True):
        super().__init__()
        self.batch_size_per_image = batch_size_per_image
        self.positive_fraction = positive_fraction
        self.num_classes = num_classes
        self.proposal_matcher = proposal_matcher
        self.proposal_append_gt = proposal_append_gt

    @classmethod
    def from_config(cls, cfg):
        return {
            "batch_size_per_image": cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE,
            "positive_fraction": cfg.MODEL.ROI_HEADS.POSITIVE_FRACTION,
            "num_classes": cfg.MODEL.ROI_HEADS.NUM_CLASSES,
            "proposal_append_gt": cfg.MODEL.ROI_HEADS.PROPOSAL_APPEND_GT,
            "proposal_matcher": Matcher(cfg.MODEL.ROI_HEADS.IOU_THRESHOLDS, cfg.MODEL.ROI_HEADS.IOU_LABELS,
                                        allow_low_quality_matches=False),
        }

    def _sample_proposals(self, matched_idxs, matched_labels, gt_classes):
        """No sub-sampling in the WSL heads: every proposal is kept and labelled."""
        if gt_classes.numel() > 0:
            gt_classes = gt_classes[matched_idxs]
            gt_classes[matched_labels == 0] = self.num_classes
            gt_classes[matched_labels == -1] = -1
        else:
            gt_classes = torch.zeros_like(matched_idxs) + self.num_classes
        return torch.arange(gt_classes.shape[0], device=gt_classes.device), gt_classes

    @torch.no_grad()
    def label_and_sample_proposals(self, proposals: List[Instances], targets: List[Instances], suffix=""):
        if self.proposal_append_gt:
            raise NotImplementedError("PROPOSAL_APPEND_GT must be False for the WSL heads "
                                      "(projects/WSL/configs/Base-RCNN-DilatedC5.yaml:15)")
        out = []
        for proposals_per_image, targets_per_image in zip(proposals, targets):
            has_gt = len(targets_per_image) > 0
            match_quality_matrix = pairwise_iou(targets_per_image.gt_boxes, proposals_per_image.proposal_boxes)
            matched_idxs, matched_labels = self.proposal_matcher(match_quality_matrix)
            sampled_idxs, gt_classes = self._sample_proposals(matched_idxs, matched_labels,
                                                              targets_per_image.gt_classes)
            proposals_per_image = proposals_per_image[sampled_idxs]
            proposals_per_image.gt_classes = gt_classes
            if has_gt:
                sampled_targets = matched_idxs[sampled_idxs]
                for name, value in targets_per_image.get_fields().items():
                    if name.startswith("gt_") and name != "gt_classes":
                        proposals_per_image.set(name, value[sampled_targets])
                proposals_per_image.set("matched_gt_idx", sampled_targets)
            out.append(proposals_per_image)
        return out


@ROI_HEADS_REGISTRY.register()
class StandardROIHeads(torch.nn.Module):
    """The fully supervised box (+ mask) heads of BASELINE configs[0] — call surface of
    detectron2/modeling/roi_heads/roi_heads.py:520-875: ground truth appended to the proposals, IoU matching, 512
    sampled rois per image (25 % foreground), multi-level ROIAlignV2 -> box head -> FastRCNNOutputLayers; with
    MASK_ON, ROIAlign 14 x 14 of the foreground rois -> mask head -> per-class BCE against the matched instance's
    bitmask cropped to the roi (structures/masks.py:169-200, the same ROIAlign).  Plumbing over this repo's kernels."""

    pairwise_iou = staticmethod(pairwise_iou)      # (the rotated IoU in RROIHeads)

    def __init__(self, cfg, input_shape):
        super().__init__()
        from ...layers.shape_spec import ShapeSpec
        from ..poolers import ROIPooler
        from ..sampling import subsample_labels  # noqa: F401  (used in label_and_sample_proposals)
        from .box_head import build_box_head
        from .mask_head import build_mask_head

        h = cfg.MODEL.ROI_HEADS
        self.num_classes, self.batch_size_per_image = h.NUM_CLASSES, h.BATCH_SIZE_PER_IMAGE
        self.positive_fraction, self.proposal_append_gt = h.POSITIVE_FRACTION, h.PROPOSAL_APPEND_GT
        self.proposal_matcher = Matcher(h.IOU_THRESHOLDS, h.IOU_LABELS, allow_low_quality_matches=False)
        self.in_features = h.IN_FEATURES
        scales = tuple(1.0 / input_shape[k].stride for k in self.in_features)
        channels = {input_shape[f].channels for f in self.in_features}
        assert len(channels) == 1, channels
        c = channels.pop()
        b = cfg.MODEL.ROI_BOX_HEAD
        self.box_pooler = ROIPooler(output_size=b.POOLER_RESOLUTION, scales=scales, sampling_ratio=b.POOLER_SAMPLING_RATIO,
                                    pooler_type=b.POOLER_TYPE)
        self.box_head = build_box_head(cfg, ShapeSpec(channels=c, height=b.POOLER_RESOLUTION, width=b.POOLER_RESOLUTION))
        self.box_predictor = self._box_predictor(cfg, self.box_head.output_shape)
        self.mask_on = cfg.MODEL.MASK_ON
        self.train_on_pred_boxes = b.TRAIN_ON_PRED_BOXES
        if self.mask_on:
            m = cfg.MODEL.ROI_MASK_HEAD
            if m.POOLER_TYPE:
                self.mask_pooler = ROIPooler(output_size=m.POOLER_RESOLUTION, scales=scales,
                                             sampling_ratio=m.POOLER_SAMPLING_RATIO, pooler_type=m.POOLER_TYPE)
                self.mask_head = build_mask_head(cfg, ShapeSpec(channels=c, width=m.POOLER_RESOLUTION,
                                                                height=m.POOLER_RESOLUTION))
            else:
                # detectron2/modeling/roi_heads/roi_heads.py:630-641: no roi pooling, the head (PointRendMaskHead)
                # reads the image-level features itself and is given their shapes
                self.mask_pooler = None
                self.mask_head = build_mask_head(cfg, {f: input_shape[f] for f in self.in_features})
        self.keypoint_on = cfg.MODEL.KEYPOINT_ON
        if self.keypoint_on:
            # detectron2/modeling/roi_heads/roi_heads.py:669-697 (_init_keypoint_head); imported only here, so a model
            # without keypoints never loads the keypoint modules
            from .keypoint_head import build_keypoint_head
            k = cfg.MODEL.ROI_KEYPOINT_HEAD
            self.keypoint_pooler = ROIPooler(output_size=k.POOLER_RESOLUTION, scales=scales,
                                             sampling_ratio=k.POOLER_SAMPLING_RATIO, pooler_type=k.POOLER_TYPE)
            self.keypoint_head = build_keypoint_head(cfg, ShapeSpec(channels=c, width=k.POOLER_RESOLUTION,
                                                                    height=k.POOLER_RESOLUTION))

    def _box_predictor(self, cfg, input_shape):
        from .fast_rcnn import FastRCNNOutputLayers
        return FastRCNNOutputLayers(cfg, input_shape)

    @torch.no_grad()
    def label_and_sample_proposals(self, proposals: List[Instances], targets: List[Instances]):
        from ..proposal_generator.proposal_utils import add_ground_truth_to_proposals
        from ..sampling import subsample_labels

        if self.proposal_append_gt:
            proposals = add_ground_truth_to_proposals([t.gt_boxes for t in targets], proposals)
        out = []
        for prop, tgt in zip(proposals, targets):
            has_gt = len(tgt) > 0
            idx, lab = self.proposal_matcher(self.pairwise_iou(tgt.gt_boxes, prop.proposal_boxes))
            if has_gt:
                cls = tgt.gt_classes[idx].clone()
                cls[lab == 0] = self.num_classes
                cls[lab == -1] = -1
            else:
                cls = torch.zeros_like(idx) + self.num_classes
            pos, neg = subsample_labels(cls, self.batch_size_per_image, self.positive_fraction, self.num_classes)
            keep = torch.cat([pos, neg], dim=0)
            prop = prop[keep]
            prop.gt_classes = cls[keep]
            if has_gt:
                chosen = idx[keep]
                for name, value in tgt.get_fields().items():
                    if name.startswith("gt_") and not prop.has(name):
                        prop.set(name, value[chosen])
                prop.set("matched_gt_idx", chosen)
            out.append(prop)
        return out

    def forward(self, images, features, proposals, targets=None):
        if self.training:
            assert targets, "'targets' argument is required during training"
            proposals = self.label_and_sample_proposals(proposals, targets)
            losses = self._forward_box(features, proposals)
            if self.mask_on:
                losses.update(self._forward_mask(features, proposals, targets))
            if self.keypoint_on:
                losses.update(self._forward_keypoint(features, proposals))
            return proposals, losses
        pred = self._forward_box(features, proposals)
        return self.forward_with_given_boxes(features, pred), {}

    def _forward_box(self, features, proposals):
        feats = [features[f] for f in self.in_features]
        x = self.box_head(self.box_pooler(feats, [p.proposal_boxes for p in proposals]))
        predictions = self.box_predictor(x)
        if self.training:
            losses = self.box_predictor.losses(predictions, proposals)
            if self.train_on_pred_boxes:
                # roi_heads.py:739-746: the later heads train on the boxes this one predicts, detached
                for prop, boxes in zip(proposals, self.box_predictor.predict_boxes_for_gt_classes(predictions, proposals)):
                    prop.proposal_boxes = Boxes(boxes)
            return losses
        return self.box_predictor.inference(predictions, proposals)[0]

    @torch.no_grad()
    def forward_with_given_boxes(self, features, instances):
        if self.mask_on and self.mask_pooler is None:
            instances = self.mask_head({f: features[f] for f in self.in_features}, instances)
        elif self.mask_on:
            from .mask_head import mask_rcnn_inference
            feats = [features[f] for f in self.in_features]
            x = self.mask_pooler(feats, [i.pred_boxes for i in instances])
            mask_rcnn_inference(self.mask_head.layers(x)[0], instances)
        if self.keypoint_on:
            instances = self._forward_keypoint(features, instances)
        return instances

    def _forward_keypoint(self, features, instances):
        """detectron2/modeling/roi_heads/roi_heads.py:839-875.  Training: the foreground rois whose matched instance
        has a labelled keypoint inside the roi -> {"loss_keypoint"}; inference: `pred_keypoints` and
        `pred_keypoint_heatmaps` added to the detections."""
        feats = [features[f] for f in self.in_features]
        if self.training:
            instances, _ = select_foreground_proposals(instances, self.num_classes)
            instances = select_proposals_with_visible_keypoints(instances)
            boxes = [x.proposal_boxes for x in instances]
        else:
            boxes = [x.pred_boxes for x in instances]
        return self.keypoint_head(self.keypoint_pooler(feats, boxes), instances)

    def _forward_mask(self, features, proposals, targets):
        """Foreground rois only; the target of a roi is its matched instance's bitmask cropped to the roi at
        2 x POOLER_RESOLUTION (crop_and_resize = ROIAlign(1.0, sampling 0, aligned) >= 0.5)."""
        from .mask_head import mask_rcnn_loss

        fg, _ = select_foreground_proposals(proposals, self.num_classes)
        if self.mask_pooler is None:
            return self.mask_head({f: features[f] for f in self.in_features}, fg, targets)
        feats = [features[f] for f in self.in_features]
        logits, _ = self.mask_head.layers(self.mask_pooler(feats, [p.proposal_boxes for p in fg]))
        side = logits.shape[-1] if logits.shape[0] else 2 * self.mask_pooler.output_size[0]
        tgt = cropped_mask_targets(fg, targets, side)
        classes = torch.cat([p.gt_classes for p in fg]) if fg else logits.new_zeros(0, dtype=torch.long)
        if tgt is None:
            return {"loss_mask": logits.sum() * 0}
        return {"loss_mask": mask_rcnn_loss(logits, classes.to(torch.int64), tgt)}
