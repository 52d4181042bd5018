"""RetinaNet — call surface of detectron2/modeling/meta_arch/retinanet.py:39-616 (RetinaNet, RetinaNetHead): same
constructor keywords, from_config, attribute and state-dict names.

MI355X mapping: the head's 3x3 convolutions are MFMA launches shared across the levels; what follows them
is three library calls instead of device-op graphs over (N, R, K): anchor labelling for the batch
(retinanet_label_anchors), the focal and smooth-L1 losses with the EMA normaliser each way (retinanet_loss: reads the
head's channels-last maps where the convolutions wrote them and writes their gradients in place of a cat / gather /
one-hot chain), and per-level candidate selection + decode for every image (retinanet_candidates), followed by the
existing batched NMS per image.  Nothing is read back in training; inference reads the final counts once, at its end."""
import math
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from ...layers.batch_norm import get_norm
from ...layers.conv import planes_clear
from ...layers.postprocess import batched_nms_device
from ...layers.retinanet import retinanet_candidates, retinanet_label_anchors, retinanet_loss
from ...layers.shape_spec import ShapeSpec
from ...layers.wrappers import Conv2d, conv2d_padded
from ...structures import Boxes, ImageList, Instances
from ..anchor_generator import build_anchor_generator
from ..backbone import build_backbone
from ..box_regression import Box2BoxTransform
from ..matcher import Matcher
from ..postprocessing import detector_postprocess
from .build import META_ARCH_REGISTRY

__all__ = ["RetinaNet", "RetinaNetHead", "permute_to_N_HWA_K"]


def permute_to_N_HWA_K(tensor, K: int):
    """(N, Ai * K, H, W) -> (N, H * W * Ai, K) (retinanet.py:27-36): a view of a dense channels-last map, a copy of a
    channel slice of a padded one (the fused path reads either in place and does not come through here)."""
    assert tensor.dim() == 4, tensor.shape
    n, _, h, w = tensor.shape
    return tensor.view(n, -1, K, h, w).permute(0, 3, 4, 1, 2).reshape(n, -1, K)


@META_ARCH_REGISTRY.register()
class RetinaNet(nn.Module):
    """Built from a cfg (`RetinaNet(cfg)`, as build_model does) or from the reference's keywords."""

    def __init__(self, cfg=None, *, backbone=None, head=None, head_in_features=None, anchor_generator=None,
                 box2box_transform=None, anchor_matcher=None, num_classes=None, focal_loss_alpha=0.25,
                 focal_loss_gamma=2.0, smooth_l1_beta=0.1, box_reg_loss_type="smooth_l1", test_score_thresh=0.05,
                 test_topk_candidates=1000, test_nms_thresh=0.5, max_detections_per_image=100, pixel_mean=None,
                 pixel_std=None, vis_period=0, input_format="BGR"):
        if cfg is not None:
            self.__init__(**self.from_config(cfg))
            return
        super().__init__()
        if box_reg_loss_type != "smooth_l1":
            raise NotImplementedError("RETINANET.BBOX_REG_LOSS_TYPE: smooth_l1 only (got %r)" % (box_reg_loss_type,))
        self.backbone, self.head, self.head_in_features = backbone, head, head_in_features
        self.anchor_generator, self.box2box_transform, self.anchor_matcher = anchor_generator, box2box_transform, anchor_matcher
        self.num_classes = num_classes
        self.focal_loss_alpha, self.focal_loss_gamma = focal_loss_alpha, focal_loss_gamma
        self.smooth_l1_beta, self.box_reg_loss_type = smooth_l1_beta, box_reg_loss_type
        self.test_score_thresh, self.test_topk_candidates = test_score_thresh, test_topk_candidates
        self.test_nms_thresh, self.max_detections_per_image = test_nms_thresh, max_detections_per_image
        self.vis_period, self.input_format = vis_period, input_format
        self.register_buffer("pixel_mean", torch.Tensor(pixel_mean).view(-1, 1, 1))
        self.register_buffer("pixel_std", torch.Tensor(pixel_std).view(-1, 1, 1))
        # the EMA of the number of foreground anchors (retinanet.py:143-150), kept as one fp64 value on the device and
        # updated by the loss kernel: never read back.  Not persistent: the state dict has the reference's keys.
        self.register_buffer("loss_normalizer", torch.full((1,), 100.0, dtype=torch.float64), persistent=False)
        self.loss_normalizer_momentum = 0.9

    @classmethod
    def from_config(cls, cfg):
        r = cfg.MODEL.RETINANET
        if r.BBOX_REG_LOSS_TYPE != "smooth_l1":
            raise NotImplementedError("RETINANET.BBOX_REG_LOSS_TYPE: smooth_l1 only (got %r)" % (r.BBOX_REG_LOSS_TYPE,))
        backbone = build_backbone(cfg)
        shapes = backbone.output_shape()
        feature_shapes = [shapes[f] for f in r.IN_FEATURES]
        return {
            "backbone": backbone,
            "head": RetinaNetHead(cfg, feature_shapes),
            "anchor_generator": build_anchor_generator(cfg, feature_shapes),
            "box2box_transform": Box2BoxTransform(weights=r.BBOX_REG_WEIGHTS),
            "anchor_matcher": Matcher(r.IOU_THRESHOLDS, r.IOU_LABELS, allow_low_quality_matches=True),
            "pixel_mean": cfg.MODEL.PIXEL_MEAN,
            "pixel_std": cfg.MODEL.PIXEL_STD,
            "num_classes": r.NUM_CLASSES,
            "head_in_features": r.IN_FEATURES,
            "focal_loss_alpha": r.FOCAL_LOSS_ALPHA,
            "focal_loss_gamma": r.FOCAL_LOSS_GAMMA,
            "smooth_l1_beta": r.SMOOTH_L1_LOSS_BETA,
            "box_reg_loss_type": r.BBOX_REG_LOSS_TYPE,
            "test_score_thresh": r.SCORE_THRESH_TEST,
            "test_topk_candidates": r.TOPK_CANDIDATES_TEST,
            "test_nms_thresh": r.NMS_THRESH_TEST,
            "max_detections_per_image": cfg.TEST.DETECTIONS_PER_IMAGE,
            "vis_period": cfg.VIS_PERIOD,
            "input_format": cfg.INPUT.FORMAT,
        }

    @property
    def device(self):
        return self.pixel_mean.device

    # ------------------------------------------------------------------ forward
    def forward(self, batched_inputs: Tuple[Dict[str, torch.Tensor]]):
        planes_clear()
        images = self.preprocess_image(batched_inputs)
        features = self.backbone(images.tensor)
        features = [features[f] for f in self.head_in_features]
        anchors = self.anchor_generator(features)
        pred_logits, pred_anchor_deltas = self.head(features)      # (N, A * K, H, W) / (N, A * 4, H, W), read in place
        if self.training:
            assert "instances" in batched_inputs[0], "Instance annotations are missing in training!"
            gt_instances = [x["instances"].to(self.device) for x in batched_inputs]
            labels, matched, offsets, num_pos, gt_boxes = self._label(anchors, gt_instances)
            return self._losses(anchors, pred_logits, pred_anchor_deltas, labels, matched, gt_boxes, offsets, num_pos)
        results = self.inference(anchors, pred_logits, pred_anchor_deltas, images.image_sizes)
        processed = []
        for r, inp, size in zip(results, batched_inputs, images.image_sizes):
            processed.append({"instances": detector_postprocess(r, inp.get("height", size[0]), inp.get("width", size[1]))})
        return processed

    # ------------------------------------------------------------------ training
    def _thresholds(self):
        return self.anchor_matcher.thresholds[1:-1], self.anchor_matcher.labels

    @torch.no_grad()
    def _label(self, anchors, gt_instances):
        """One labelling call for the batch -> labels (N, R) int32, matched (N, R) int32, gt offsets, the positive
        count (device) and the concatenated gt boxes."""
        flat = Boxes.cat(anchors).tensor
        gt_boxes = torch.cat([g.gt_boxes.tensor for g in gt_instances]).to(torch.float32)
        gt_classes = torch.cat([g.gt_classes for g in gt_instances])
        thresholds, table = self._thresholds()
        labels, matched, offsets, num_pos = retinanet_label_anchors(
            flat, gt_boxes, gt_classes, [len(g) for g in gt_instances], self.num_classes, thresholds, table)
        return labels, matched, offsets, num_pos, gt_boxes

    def _losses(self, anchors, pred_logits, pred_anchor_deltas, labels, matched, gt_boxes, offsets, num_pos):
        flat = type(anchors[0]).cat(anchors).tensor
        loss_cls, loss_box_reg = retinanet_loss(
            pred_logits, pred_anchor_deltas, labels, matched, flat, gt_boxes, offsets, num_pos, self.loss_normalizer,
            self.num_classes, alpha=self.focal_loss_alpha, gamma=self.focal_loss_gamma, beta=self.smooth_l1_beta,
            weights=self.box2box_transform.weights, momentum=self.loss_normalizer_momentum, training=self.training)
        return {"loss_cls": loss_cls, "loss_box_reg": loss_box_reg}

    @torch.no_grad()
    def label_anchors(self, anchors, gt_instances):
        """-> list of N (R,) int64 label vectors in {-1, 0 .. K}, list of N (R, 4) matched gt boxes (retinanet.py:353-397),
        gathered from the fused labelling's outputs."""
        labels, matched, offsets, _, gt_boxes = self._label(anchors, gt_instances)
        out_labels, out_boxes = [], []
        flat = Boxes.cat(anchors).tensor
        start = 0
        for n, g in enumerate(gt_instances):
            out_labels.append(labels[n].to(torch.int64))
            if len(g):
                out_boxes.append(gt_boxes[start + matched[n].to(torch.int64)])
            else:
                out_boxes.append(torch.zeros_like(flat))
            start += len(g)
        return out_labels, out_boxes

    def losses(self, anchors, pred_logits, gt_labels, pred_anchor_deltas, gt_boxes):
        """The reference's call (retinanet.py:287-351): per-image label vectors and matched boxes in, the two losses
        out — through the same kernels: the (N * R, 4) matched boxes are the gt array, each anchor matched to its own
        row."""
        n, r = len(gt_labels), gt_labels[0].shape[0]
        labels = torch.stack(gt_labels).to(torch.int32)
        boxes = torch.stack(gt_boxes).reshape(n * r, 4).to(torch.float32)
        matched = torch.arange(r, dtype=torch.int32, device=labels.device).unsqueeze(0).expand(n, r).contiguous()
        offsets = torch.arange(n + 1, dtype=torch.int32, device=labels.device) * r
        num_pos = ((labels >= 0) & (labels != self.num_classes)).sum().to(torch.int32).reshape(1)
        return self._losses(anchors, pred_logits, pred_anchor_deltas, labels, matched, boxes, offsets, num_pos)

    # ------------------------------------------------------------------ inference
    @torch.no_grad()
    def inference(self, anchors: List[Boxes], pred_logits: List[torch.Tensor], pred_anchor_deltas: List[torch.Tensor],
                  image_sizes: List[Tuple[int, int]]):
        """Per-level (N, A * K, H, W) maps or (N, HWA, K) views -> list[Instances].  One candidate call for the batch,
        one batched NMS per image on the padded slots, one read-back of the N final counts."""
        flat = type(anchors[0]).cat(anchors).tensor
        topk, levels = int(self.test_topk_candidates), len(pred_logits)
        boxes, scores, classes, _ = retinanet_candidates(
            pred_logits, pred_anchor_deltas, flat, self.num_classes, self.test_score_thresh, topk,
            weights=self.box2box_transform.weights, scale_clamp=self.box2box_transform.scale_clamp)
        keeps, nums = [], []
        for n in range(len(image_sizes)):
            keep, num, _ = batched_nms_device(boxes[n], scores[n], classes[n], self.test_nms_thresh, self.num_classes,
                                              levels * topk, coordinate_trick=2)
            keeps.append(keep)
            nums.append(num)
        counts = torch.cat(nums).clamp(max=int(self.max_detections_per_image)).tolist() if nums else []
        results = []
        for n, (size, keep, c) in enumerate(zip(image_sizes, keeps, counts)):
            keep = keep[:c]
            r = Instances(size)
            r.pred_boxes = Boxes(boxes[n][keep])
            r.scores = scores[n][keep]
            r.pred_classes = classes[n][keep]
            results.append(r)
        return results

    def inference_single_image(self, anchors: List[Boxes], box_cls: List[torch.Tensor], box_delta: List[torch.Tensor],
                               image_size: Tuple[int, int]):
        """One image: box_cls (HWA, K) and box_delta (HWA, 4) per level (retinanet.py:427-493)."""
        return self.inference(anchors, [x.unsqueeze(0) for x in box_cls], [x.unsqueeze(0) for x in box_delta],
                              [image_size])[0]

    def preprocess_image(self, batched_inputs: Tuple[Dict[str, torch.Tensor]]):
        images = [(x["image"].to(self.device) - self.pixel_mean) / self.pixel_std for x in batched_inputs]
        return ImageList.from_tensors(images, self.backbone.size_divisibility, channels_last=True)


class RetinaNetHead(nn.Module):
    """Two towers of 3x3 convolutions + ReLU shared by all levels, then cls_score (A * K) and bbox_pred (A * 4)
    (retinanet.py:505-615).  Built from (cfg, input_shape) or from the reference's keywords."""

    def __init__(self, cfg=None, input_shape: List[ShapeSpec] = None, *, num_classes=None, num_anchors=None,
                 conv_dims: List[int] = None, norm="", prior_prob=0.01):
        if cfg is not None:
            self.__init__(**self.from_config(cfg, input_shape))
            return
        super().__init__()
        cls_subnet, bbox_subnet = [], []
        for in_channels, out_channels in zip([input_shape[0].channels] + list(conv_dims), conv_dims):
            for tower in (cls_subnet, bbox_subnet):
                if norm:
                    tower += [Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1),
                              get_norm(norm, out_channels), nn.ReLU()]
                else:   # the ReLU in the convolution's epilogue; the slot keeps the reference's indices 0, 2, 4, 6
                    tower += [Conv2d(in_channels, out_channels, kernel_size=3, stride=1, padding=1, activation=F.relu),
                              nn.Identity()]
        self.cls_subnet = nn.Sequential(*cls_subnet)
        self.bbox_subnet = nn.Sequential(*bbox_subnet)
        self.cls_score = Conv2d(conv_dims[-1], num_anchors * num_classes, kernel_size=3, stride=1, padding=1)
        self.bbox_pred = Conv2d(conv_dims[-1], num_anchors * 4, kernel_size=3, stride=1, padding=1)
        for modules in (self.cls_subnet, self.bbox_subnet, self.cls_score, self.bbox_pred):
            for layer in modules.modules():
                if isinstance(layer, nn.Conv2d):
                    nn.init.normal_(layer.weight, mean=0, std=0.01)
                    nn.init.constant_(layer.bias, 0)
        nn.init.constant_(self.cls_score.bias, -(math.log((1 - prior_prob) / prior_prob)))

    @classmethod
    def from_config(cls, cfg, input_shape: List[ShapeSpec]):
        num_anchors = build_anchor_generator(cfg, input_shape).num_cell_anchors
        assert len(set(num_anchors)) == 1, "Using different number of anchors between levels is not currently supported!"
        r = cfg.MODEL.RETINANET
        return {"input_shape": input_shape, "num_classes": r.NUM_CLASSES,
                "conv_dims": [input_shape[0].channels] * r.NUM_CONVS, "prior_prob": r.PRIOR_PROB, "norm": r.NORM,
                "num_anchors": num_anchors[0]}

    def forward(self, features: List[torch.Tensor]):
        """-> logits (N, A * K, Hi, Wi) and bbox_reg (N, A * 4, Hi, Wi) per level, channels-last (bbox_reg a channel
        slice of a map padded to a multiple of 8: layers/wrappers.py conv2d_padded)."""
        logits, bbox_reg = [], []
        for feature in features:
            logits.append(conv2d_padded(self.cls_score, self.cls_subnet(feature)))
            bbox_reg.append(conv2d_padded(self.bbox_pred, self.bbox_subnet(feature)))
        return logits, bbox_reg
