"""Keypoint head — surface of detectron2/modeling/roi_heads/keypoint_head.py: the registry, keypoint_rcnn_loss (:40-96),
keypoint_rcnn_inference (:99-132), BaseKeypointRCNNHead (:135-211) and KRCNNConvDeconvUpsampleHead (:217-272) with the
reference's module names and state-dict shapes.

The eight 3x3 + ReLU layers are `Conv2d`s on the contraction kernels.  `score_lowres` (ConvTranspose2d 4x4, stride 2,
padding 1) runs as a 3x3 convolution to 4 K parity-major channels on the same kernels; its pixel shuffle and the x2
bilinear up-sampling are one pass that writes contiguous (R, K, S, S) logits (jtsm_amd/csrc/keypoint.hip).  Targets,
loss and decode are library calls on those rows; nothing between the matched ground-truth keypoints and the scalar
loss, or between the logits and `pred_keypoints`, is read back to the host."""
from typing import List

import torch
import torch.nn.functional as F
from torch import nn

from ...layers.conv import conv2d_fused
from ...layers.keypoint import keypoint_loss, keypoint_upsample, transposed4x4_as_conv3x3
from ...layers.wrappers import Conv2d, cat
from ...structures import Instances, heatmaps_to_keypoints
from ...utils.registry import Registry

__all__ = ["ROI_KEYPOINT_HEAD_REGISTRY", "build_keypoint_head", "keypoint_rcnn_loss", "keypoint_rcnn_inference",
           "BaseKeypointRCNNHead", "KRCNNConvDeconvUpsampleHead"]

ROI_KEYPOINT_HEAD_REGISTRY = Registry("ROI_KEYPOINT_HEAD")


def build_keypoint_head(cfg, input_shape):
    return ROI_KEYPOINT_HEAD_REGISTRY.get(cfg.MODEL.ROI_KEYPOINT_HEAD.NAME)(cfg, input_shape)


def keypoint_rcnn_loss(pred_keypoint_logits, instances: List[Instances], normalizer):
    """pred_keypoint_logits (N, K, S, S) in 1:1 correspondence with the instances' rows (`proposal_boxes`,
    `gt_keypoints`); normalizer None: the number of visible keypoints.  Soft-max cross-entropy over space, summed over
    the valid keypoints; a batch without one gives 0 with a zero gradient (the reference's `logits.sum() * 0`; its
    `kpts_num_skipped_batches` counter would need the count on the host and is not kept)."""
    side = pred_keypoint_logits.shape[2]
    targets, valid = [], []
    for per_image in instances:
        if len(per_image) == 0:
            continue
        t, v = per_image.gt_keypoints.to_heatmap(per_image.proposal_boxes.tensor, side)
        targets.append(t.view(-1))
        valid.append(v.view(-1))
    if not targets:
        return pred_keypoint_logits.sum() * 0
    return keypoint_loss(pred_keypoint_logits, cat(targets, dim=0), cat(valid, dim=0), normalizer)


@torch.no_grad()
def keypoint_rcnn_inference(pred_keypoint_logits: torch.Tensor, pred_instances: List[Instances]):
    """Adds `pred_keypoints` (Ri, K, 3) = x, y, score and `pred_keypoint_heatmaps` (Ri, K, S, S) to each image's
    instances."""
    boxes = cat([b.pred_boxes.tensor for b in pred_instances], dim=0)
    logits = pred_keypoint_logits.detach()
    results = heatmaps_to_keypoints(logits, boxes.detach())
    counts = [len(i) for i in pred_instances]
    results = results[:, :, [0, 1, 3]].split(counts, dim=0)
    for points, heatmaps, per_image in zip(results, logits.split(counts, dim=0), pred_instances):
        per_image.pred_keypoints = points
        per_image.pred_keypoint_heatmaps = heatmaps


class BaseKeypointRCNNHead(nn.Module):
    """Losses and inference of Sec. 5 of Mask R-CNN.  Built from (cfg, input_shape) or from keywords."""

    def __init__(self, *, num_keypoints, loss_weight=1.0, loss_normalizer=1.0):
        super().__init__()
        self.num_keypoints = num_keypoints
        self.loss_weight = loss_weight
        assert loss_normalizer == "visible" or isinstance(loss_normalizer, float), loss_normalizer
        self.loss_normalizer = loss_normalizer

    @classmethod
    def from_config(cls, cfg, input_shape):
        k = cfg.MODEL.ROI_KEYPOINT_HEAD
        ret = {"loss_weight": k.LOSS_WEIGHT, "num_keypoints": k.NUM_KEYPOINTS}
        if k.NORMALIZE_LOSS_BY_VISIBLE_KEYPOINTS:
            ret["loss_normalizer"] = "visible"
        else:
            ret["loss_normalizer"] = float(k.NUM_KEYPOINTS * cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE *
                                           cfg.MODEL.ROI_HEADS.POSITIVE_FRACTION)
        return ret

    def forward(self, x, instances: List[Instances]):
        x = self.layers(x)
        if self.training:
            normalizer = None if self.loss_normalizer == "visible" else len(instances) * self.loss_normalizer
            return {"loss_keypoint": keypoint_rcnn_loss(x, instances, normalizer=normalizer) * self.loss_weight}
        keypoint_rcnn_inference(x, instances)
        return instances

    def layers(self, x):
        raise NotImplementedError


class _ScoreLowres(nn.ConvTranspose2d):
    """ConvTranspose2d(in, K, 4, stride 2, padding 1) with the reference's parameters (weight (in, K, 4, 4), bias
    (K,)).  `parity_planes` is the layer before its pixel shuffle: (R, 4 K padded, H, W) channels-last, from the 3x3
    convolution the transposed one equals (layers/keypoint.py: transposed4x4_as_conv3x3)."""

    def parity_planes(self, x):
        w3, b3 = transposed4x4_as_conv3x3(self.weight, self.bias)
        return conv2d_fused(x, w3, None, b3, None, 1, 1, 1, False, True, emit_planes=False)

    def forward(self, x):
        z = self.parity_planes(x)
        r, _, h, w = z.shape
        k = self.out_channels
        return z[:, :4 * k].reshape(r, 2, 2, k, h, w).permute(0, 3, 4, 1, 5, 2).reshape(r, k, 2 * h, 2 * w)


@ROI_KEYPOINT_HEAD_REGISTRY.register()
class KRCNNConvDeconvUpsampleHead(BaseKeypointRCNNHead):
    """3x3 convs + ReLU, the 4x4 transposed convolution and a x2 bilinear up-sampling: conv_fcn1..N, score_lowres."""

    def __init__(self, cfg_or_shape, input_shape=None, *, num_keypoints=None, conv_dims=None, **kwargs):
        if input_shape is not None:
            cfg = cfg_or_shape
            kwargs = dict(self.from_config(cfg, input_shape), **kwargs)
            num_keypoints = kwargs.pop("num_keypoints")
            conv_dims = cfg.MODEL.ROI_KEYPOINT_HEAD.CONV_DIMS
        else:
            input_shape = cfg_or_shape
        super().__init__(num_keypoints=num_keypoints, **kwargs)
        self.up_scale = 2.0
        in_channels = input_shape.channels
        self.conv_fcns = []
        for idx, layer_channels in enumerate(conv_dims, 1):
            conv = Conv2d(in_channels, layer_channels, 3, stride=1, padding=1, activation=F.relu)
            self.add_module("conv_fcn{}".format(idx), conv)
            self.conv_fcns.append(conv)
            in_channels = layer_channels
        self.score_lowres = _ScoreLowres(in_channels, num_keypoints, 4, stride=2, padding=1)
        for name, param in self.named_parameters():
            if "bias" in name:
                nn.init.constant_(param, 0)
            elif "weight" in name:
                nn.init.kaiming_normal_(param, mode="fan_out", nonlinearity="relu")

    def layers(self, x):
        for conv in self.conv_fcns:
            x = conv(x)
        return keypoint_upsample(self.score_lowres.parity_planes(x), self.num_keypoints)
