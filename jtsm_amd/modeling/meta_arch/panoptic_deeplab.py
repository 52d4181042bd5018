"""PanopticDeepLab, PanopticDeepLabSemSegHead, PanopticDeepLabInsEmbedHead — module names, constructor keywords,
from_config and initialisation of projects/Panoptic-DeepLab/panoptic_deeplab/panoptic_seg.py:29-561, so that a reference
state dict loads.

MI355X mapping: both heads are DeepLabV3PlusHead decoders (meta_arch/deeplab.py) followed by two 3x3 convolutions and a
1x1 predictor, all contraction launches with the fused batch norm + ReLU.  The semantic loss is deeplab_cross_entropy
with the per-pixel weights (csrc/deeplab_loss.hip); the centre and offset losses read the stride-4 predictions in place
and never materialise the up-sampled maps (csrc/panoptic_deeplab.hip).  Inference up-samples the three maps, passes them
through sem_seg_postprocess and then through ONE chain of launches per image (layers/panoptic_deeplab.py:
panoptic_deeplab_postprocess) that leaves the panoptic map, the segment table and the instance rows on the device: no
host loop over instances, classes or segments.

Differences from the reference, all declared: thing ids and label_divisor are constructor keywords (this package has no
metadata catalogue; the Cityscapes values are the defaults for cityscapes_fine_panoptic_*); "panoptic_seg" is (int32
map with every id + 1 so that void is 0, SegmentsInfo with the device table) — what the reference's evaluator makes of
the label_divisor form before it scores it; use_depthwise_separable_conv is not built."""
from typing import Callable, Dict, List, Union

import torch
import torch.nn.functional as F
from torch import nn

from ...layers.aspp import c2_xavier_fill
from ...layers.batch_norm import get_norm
from ...layers.shape_spec import ShapeSpec
from ...layers.wrappers import Conv2d
from ...utils.registry import Registry
from .build import META_ARCH_REGISTRY
from .deeplab import _LOSS_TYPES, DeepLabV3PlusHead, _predict, _predictor, _segmentation_loss
from .panoptic_fpn import SegmentsInfo
from .semantic_seg import SEM_SEG_HEADS_REGISTRY, _upsample_logits, build_sem_seg_head

__all__ = ["PanopticDeepLab", "INS_EMBED_BRANCHES_REGISTRY", "build_ins_embed_branch", "PanopticDeepLabSemSegHead",
           "PanopticDeepLabInsEmbedHead"]

INS_EMBED_BRANCHES_REGISTRY = Registry("INS_EMBED_BRANCHES")

# cityscapes_fine_panoptic_*: the contiguous ids of person .. bicycle among the 19 classes, and the dataset's divisor
CITYSCAPES_THING_IDS = tuple(range(11, 19))
CITYSCAPES_LABEL_DIVISOR = 1000


def _two_convs(in_channels, mid_channels, out_channels, norm):
    """The `head` in front of a predictor: two 3x3 convolutions with norm and ReLU, c2_xavier_fill."""
    use_bias = norm == ""
    seq = nn.Sequential(
        Conv2d(in_channels, mid_channels, kernel_size=3, padding=1, bias=use_bias, norm=get_norm(norm, mid_channels),
               activation=F.relu),
        Conv2d(mid_channels, out_channels, kernel_size=3, padding=1, bias=use_bias, norm=get_norm(norm, out_channels),
               activation=F.relu))
    c2_xavier_fill(seq[0])
    c2_xavier_fill(seq[1])
    return seq


@SEM_SEG_HEADS_REGISTRY.register()
class PanopticDeepLabSemSegHead(DeepLabV3PlusHead):
    """PanopticDeepLabSemSegHead(cfg, input_shape) or the reference's keyword constructor."""

    def _build(self, input_shape: Dict[str, ShapeSpec], *, decoder_channels: List[int], norm: Union[str, Callable],
               head_channels: int, loss_weight: float, loss_type: str, loss_top_k: float, ignore_value: int,
               num_classes: int, **kwargs):
        super()._build(input_shape, decoder_channels=decoder_channels, norm=norm, ignore_value=ignore_value, **kwargs)
        assert self.decoder_only
        self.loss_weight, self.loss_type, self.loss_top_k = loss_weight, loss_type, loss_top_k
        self.head = _two_convs(decoder_channels[0], decoder_channels[0], head_channels, norm)
        self.predictor = _predictor(head_channels, num_classes)
        if loss_type not in _LOSS_TYPES:
            raise ValueError("Unexpected loss type: %s" % loss_type)

    @classmethod
    def from_config(cls, cfg, input_shape):
        ret = super().from_config(cfg, input_shape)
        ret["head_channels"] = cfg.MODEL.SEM_SEG_HEAD.HEAD_CHANNELS
        ret["loss_top_k"] = cfg.MODEL.SEM_SEG_HEAD.LOSS_TOP_K
        return ret

    def forward(self, features, targets=None, weights=None):
        """Training: (None, losses); inference: ((N, C, H, W) logits, {})."""
        y = self.layers(features)
        if self.training:
            return None, self.losses(y, targets, weights)
        return _upsample_logits(y, self.common_stride), {}

    def layers(self, features):
        y = super().layers(features)
        return _predict(self.predictor, self.head(y))

    def losses(self, predictions, targets, weights=None):
        return _segmentation_loss(predictions, targets, self.common_stride, self.ignore_value, self.loss_type,
                                  self.loss_weight, self.loss_top_k, weights)


def build_ins_embed_branch(cfg, input_shape):
    """The instance embedding branch named by cfg.MODEL.INS_EMBED_HEAD.NAME."""
    return INS_EMBED_BRANCHES_REGISTRY.get(cfg.MODEL.INS_EMBED_HEAD.NAME)(cfg, input_shape)


@INS_EMBED_BRANCHES_REGISTRY.register()
class PanopticDeepLabInsEmbedHead(DeepLabV3PlusHead):
    """PanopticDeepLabInsEmbedHead(cfg, input_shape) or the reference's keyword constructor."""

    def _build(self, input_shape: Dict[str, ShapeSpec], *, decoder_channels: List[int], norm: Union[str, Callable],
               head_channels: int, center_loss_weight: float, offset_loss_weight: float, **kwargs):
        super()._build(input_shape, decoder_channels=decoder_channels, norm=norm, **kwargs)
        assert self.decoder_only
        self.center_loss_weight, self.offset_loss_weight = center_loss_weight, offset_loss_weight
        self.center_head = _two_convs(decoder_channels[0], decoder_channels[0], head_channels, norm)
        self.center_predictor = _predictor(head_channels, 1)
        self.offset_head = _two_convs(decoder_channels[0], decoder_channels[0], head_channels, norm)
        self.offset_predictor = _predictor(head_channels, 2)

    @classmethod
    def from_config(cls, cfg, input_shape):
        head = cfg.MODEL.INS_EMBED_HEAD
        train_size = None
        if cfg.INPUT.CROP.ENABLED:
            assert cfg.INPUT.CROP.TYPE == "absolute"
            train_size = cfg.INPUT.CROP.SIZE
        decoder_channels = [head.CONVS_DIM] * (len(head.IN_FEATURES) - 1) + [head.ASPP_CHANNELS]
        return dict(input_shape=input_shape, in_features=head.IN_FEATURES, project_channels=head.PROJECT_CHANNELS,
                    aspp_dilations=head.ASPP_DILATIONS, aspp_dropout=head.ASPP_DROPOUT,
                    decoder_channels=decoder_channels, common_stride=head.COMMON_STRIDE, norm=head.NORM,
                    train_size=train_size, head_channels=head.HEAD_CHANNELS,
                    center_loss_weight=head.CENTER_LOSS_WEIGHT, offset_loss_weight=head.OFFSET_LOSS_WEIGHT,
                    use_depthwise_separable_conv=cfg.MODEL.SEM_SEG_HEAD.USE_DEPTHWISE_SEPARABLE_CONV)

    def forward(self, features, center_targets=None, center_weights=None, offset_targets=None, offset_weights=None):
        """Training: (None, None, centre losses, offset losses); inference: (centre (N,1,H,W), offset (N,2,H,W) in
        pixels of the full resolution, {}, {})."""
        center, offset = self.layers(features)
        if self.training:
            return (None, None, self.center_losses(center, center_targets, center_weights),
                    self.offset_losses(offset, offset_targets, offset_weights))
        return (_upsample_logits(center, self.common_stride),
                _upsample_logits(offset, self.common_stride) * self.common_stride, {}, {})

    def layers(self, features):
        y = super().layers(features)
        center = _predict(self.center_predictor, self.center_head(y))
        offset = _predict(self.offset_predictor, self.offset_head(y))
        return center, offset

    def _stride(self):
        if self.common_stride != int(self.common_stride):
            raise NotImplementedError("centre / offset losses: an integer stride only")
        return int(self.common_stride)

    def center_losses(self, predictions, targets, weights):
        from ...layers.panoptic_deeplab import center_loss
        loss = center_loss(predictions.float(), targets, weights, self._stride())
        return {"loss_center": loss * self.center_loss_weight}

    def offset_losses(self, predictions, targets, weights):
        from ...layers.panoptic_deeplab import offset_loss
        loss = offset_loss(predictions.float(), targets, weights, self._stride())
        return {"loss_offset": loss * self.offset_loss_weight}


@META_ARCH_REGISTRY.register()
class PanopticDeepLab(nn.Module):
    """PanopticDeepLab(cfg, thing_ids=None, label_divisor=None): thing_ids are the contiguous ids of the thing classes,
    label_divisor the dataset's (panoptic id = class * label_divisor + instance id)."""

    def __init__(self, cfg, thing_ids=None, label_divisor=None):
        super().__init__()
        from ..backbone import build_backbone
        self.backbone = build_backbone(cfg)
        self.sem_seg_head = build_sem_seg_head(cfg, self.backbone.output_shape())
        self.ins_embed_head = build_ins_embed_branch(cfg, self.backbone.output_shape())
        self.register_buffer("pixel_mean", torch.Tensor(cfg.MODEL.PIXEL_MEAN).view(-1, 1, 1))
        self.register_buffer("pixel_std", torch.Tensor(cfg.MODEL.PIXEL_STD).view(-1, 1, 1))
        train = cfg.DATASETS.TRAIN[0] if len(cfg.DATASETS.TRAIN) else ""
        if thing_ids is None or label_divisor is None:
            if not str(train).startswith("cityscapes_fine_panoptic_"):
                raise ValueError("PanopticDeepLab: thing_ids and label_divisor are needed for the dataset %r (only "
                                 "cityscapes_fine_panoptic_* has defaults here)" % (train,))
            thing_ids = CITYSCAPES_THING_IDS if thing_ids is None else thing_ids
            label_divisor = CITYSCAPES_LABEL_DIVISOR if label_divisor is None else label_divisor
        self.thing_ids, self.label_divisor = tuple(int(i) for i in thing_ids), int(label_divisor)
        pdl = cfg.MODEL.PANOPTIC_DEEPLAB
        self.stuff_area, self.threshold = pdl.STUFF_AREA, pdl.CENTER_THRESHOLD
        self.nms_kernel, self.top_k = pdl.NMS_KERNEL, pdl.TOP_K_INSTANCE
        self.predict_instances = pdl.PREDICT_INSTANCES
        self.use_depthwise_separable_conv = pdl.USE_DEPTHWISE_SEPARABLE_CONV
        assert cfg.MODEL.SEM_SEG_HEAD.USE_DEPTHWISE_SEPARABLE_CONV == pdl.USE_DEPTHWISE_SEPARABLE_CONV

    @property
    def device(self):
        return self.pixel_mean.device

    def _batch(self, batched_inputs, key, pad_value=0.0):
        from ...structures import ImageList
        return ImageList.from_tensors([x[key].to(self.device) for x in batched_inputs],
                                      self.backbone.size_divisibility, pad_value).tensor

    def forward(self, batched_inputs):
        """batched_inputs: dicts with "image" (C,H,W); in training "sem_seg" (H,W), "sem_seg_weights" (H,W), "center"
        (H,W), "center_weights" (1,H,W), "offset" (2,H,W), "offset_weights" (1,H,W) as PanopticDeepLabTargetGenerator
        makes them; optionally the output "height" / "width".  Training: the loss dict.  Inference: per image "sem_seg"
        (C,H,W) logits, "panoptic_seg" ((H,W) int32 map, SegmentsInfo), and with PREDICT_INSTANCES "instances"."""
        from ...layers.conv import planes_clear
        from ...structures import ImageList
        planes_clear()
        images = [(x["image"].to(self.device) - self.pixel_mean) / self.pixel_std for x in batched_inputs]
        images = ImageList.from_tensors(images, self.backbone.size_divisibility, channels_last=True)
        features = self.backbone(images.tensor)
        losses = {}
        targets = weights = None
        if "sem_seg" in batched_inputs[0]:
            targets = self._batch(batched_inputs, "sem_seg", self.sem_seg_head.ignore_value)
            if "sem_seg_weights" in batched_inputs[0]:
                weights = self._batch(batched_inputs, "sem_seg_weights")
        sem_seg_results, sem_seg_losses = self.sem_seg_head(features, targets, weights)
        losses.update(sem_seg_losses)
        center_targets = center_weights = offset_targets = offset_weights = None
        if "center" in batched_inputs[0] and "offset" in batched_inputs[0]:
            center_targets = self._batch(batched_inputs, "center").unsqueeze(1)
            center_weights = self._batch(batched_inputs, "center_weights")
            offset_targets = self._batch(batched_inputs, "offset")
            offset_weights = self._batch(batched_inputs, "offset_weights")
        center_results, offset_results, center_losses, offset_losses = self.ins_embed_head(
            features, center_targets, center_weights, offset_targets, offset_weights)
        losses.update(center_losses)
        losses.update(offset_losses)
        if self.training:
            return losses
        return [self._inference(r, c, o, inp, size) for r, c, o, inp, size in
                zip(sem_seg_results, center_results, offset_results, batched_inputs, images.image_sizes)]

    @torch.no_grad()
    def _inference(self, sem_seg_result, center_result, offset_result, inp, image_size):
        from ...layers.panoptic_deeplab import panoptic_deeplab_postprocess
        from ...structures import Boxes, Instances
        from ..postprocessing import sem_seg_postprocess
        height, width = inp.get("height", image_size[0]), inp.get("width", image_size[1])
        r = sem_seg_postprocess(sem_seg_result, image_size, height, width)
        c = sem_seg_postprocess(center_result, image_size, height, width)
        o = sem_seg_postprocess(offset_result, image_size, height, width)
        post = panoptic_deeplab_postprocess(r, c, o, self.thing_ids, self.label_divisor, self.stuff_area,
                                            self.threshold, self.nms_kernel, self.top_k, void_label=-1, id_offset=1)
        info = SegmentsInfo(table=post["table"])
        for sid, isthing, category, inst, area in post["rows"]:
            seg = {"id": sid, "isthing": bool(isthing), "category_id": category, "area": area}
            if isthing:
                seg["instance_id"] = inst
            info.append(seg)
        out = {"sem_seg": r, "panoptic_seg": (post["panoptic"], info)}
        rows = post["instances"]
        if self.predict_instances and rows.shape[0] > 0:
            things = post["table"][:rows.shape[0]]
            instances = Instances((height, width))
            instances.pred_classes = things[:, 2].to(torch.int64)
            instances.pred_masks = post["panoptic"].unsqueeze(0) == things[:, 0].view(-1, 1, 1)
            instances.scores = rows[:, 4] * rows[:, 5]          # mean semantic probability x centre heat
            instances.pred_boxes = Boxes(rows[:, :4].contiguous())
            out["instances"] = instances
        return out
