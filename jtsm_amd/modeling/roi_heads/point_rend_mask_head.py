"""PointRend mask head — surface of projects/PointRend/point_rend/mask_head.py:48-275 (CoarseMaskHead,
PointRendMaskHead) and roi_heads.py (PointRendROIHeads), on the operators of layers/point_rend.py.

No roi pooling: the head reads the image-level feature maps.  The coarse head's 14 x 14 regular grid is one gather in
space-to-depth row order, so `reduce_spatial_dim_conv` (2x2, stride 2) is a contraction with K = 4C; training samples
the point head's inputs for all rois, levels and the coarse logits in one gather into one row buffer; inference carries
the predicted class's channel only through the subdivision steps."""
import logging

import torch
from torch import nn

from ...layers import grad_fan
from ...layers import point_rend as PR
from ...layers.shape_spec import ShapeSpec
from ...layers.wrappers import cat
from .mask_head import ROI_MASK_HEAD_REGISTRY, mask_rcnn_loss
from .point_head import build_point_head, contraction_rows
from .roi_heads import ROI_HEADS_REGISTRY, StandardROIHeads


@ROI_MASK_HEAD_REGISTRY.register()
class CoarseMaskHead(nn.Module):
    """mask_head.py:48-129: [1x1 conv to CONV_DIM if the input is wider] -> 2x2 / stride-2 conv -> NUM_FC x FC -> the
    (R, C, S, S) prediction.  Parameter names and shapes are the reference's; `layers_rows` takes the gathered grid in
    space-to-depth row order, `layers` the reference's (R, C, H, W) features."""

    def __init__(self, cfg, input_shape):
        super().__init__()
        m = cfg.MODEL.ROI_MASK_HEAD
        self.num_classes = cfg.MODEL.ROI_HEADS.NUM_CLASSES
        conv_dim, self.fc_dim = m.CONV_DIM, m.FC_DIM
        self.output_side_resolution = m.OUTPUT_SIDE_RESOLUTION
        self.input_channels, self.input_h, self.input_w = input_shape.channels, input_shape.height, input_shape.width
        if self.input_h % 2 or self.input_w % 2:
            raise NotImplementedError("CoarseMaskHead: an even pooler resolution (2x2 / stride-2 reduction)")
        self.conv_layers = []
        if self.input_channels > conv_dim:
            self.reduce_channel_dim_conv = nn.Conv2d(self.input_channels, conv_dim, kernel_size=1, bias=True)
            self.conv_layers.append(self.reduce_channel_dim_conv)
        self.reduce_spatial_dim_conv = nn.Conv2d(conv_dim, conv_dim, kernel_size=2, stride=2, padding=0, bias=True)
        self.conv_layers.append(self.reduce_spatial_dim_conv)
        input_dim = conv_dim * self.input_h * self.input_w // 4
        self.fcs = []
        for k in range(m.NUM_FC):
            fc = nn.Linear(input_dim, self.fc_dim)
            self.add_module("coarse_mask_fc{}".format(k + 1), fc)
            self.fcs.append(fc)
            input_dim = self.fc_dim
        self.prediction = nn.Linear(self.fc_dim, self.num_classes * self.output_side_resolution ** 2)
        nn.init.normal_(self.prediction.weight, std=0.001)
        nn.init.constant_(self.prediction.bias, 0)
        for layer in self.conv_layers:        # c2_msra_fill
            nn.init.kaiming_normal_(layer.weight, mode="fan_out", nonlinearity="relu")
            nn.init.constant_(layer.bias, 0)
        for layer in self.fcs:                # c2_xavier_fill
            nn.init.kaiming_uniform_(layer.weight, a=1)
            nn.init.constant_(layer.bias, 0)

    def layers_rows(self, rows, num_rois):
        """rows (R * H * W, C) in the order (r, by, bx, dy, dx): four consecutive rows are one 2x2 window."""
        if self.input_channels > self.reduce_spatial_dim_conv.in_channels:
            c = self.reduce_channel_dim_conv
            rows = contraction_rows(rows, c.weight.flatten(1), c.bias, True)
        c = self.reduce_spatial_dim_conv
        cells = self.input_h * self.input_w // 4
        # (O, C, 2, 2) -> (O, 2, 2, C): the window's (dy, dx, channel) order, a view of the parameter made contiguous
        w = c.weight.permute(0, 2, 3, 1).reshape(c.out_channels, -1)
        x = contraction_rows(rows.reshape(num_rois * cells, -1), w, c.bias, True)              # (R * cells, O)
        # torch.flatten(x, 1) of the reference's (R, O, h, w): channel-major
        x = x.view(num_rois, cells, c.out_channels).permute(0, 2, 1).reshape(num_rois, -1)
        for layer in self.fcs:
            x = contraction_rows(x, layer.weight, layer.bias, True)
        x = contraction_rows(x, self.prediction.weight, self.prediction.bias, False)
        return x.view(num_rois, self.num_classes, self.output_side_resolution, self.output_side_resolution)

    def layers(self, x):
        n = x.shape[0]
        x = x.reshape(n, self.input_channels, self.input_h // 2, 2, self.input_w // 2, 2)
        rows = x.permute(0, 2, 4, 3, 5, 1).reshape(n * self.input_h * self.input_w, self.input_channels)
        return self.layers_rows(rows, n)


@ROI_MASK_HEAD_REGISTRY.register()
class PointRendMaskHead(nn.Module):
    """mask_head.py:132-275.  forward(features, instances[, targets]): `targets` (training) are the images' ground
    truth, whose (G, H, W) bitmasks the point loss samples through each proposal's `matched_gt_idx`."""

    def __init__(self, cfg, input_shape):
        super().__init__()
        m = cfg.MODEL.ROI_MASK_HEAD
        self.mask_coarse_in_features = list(m.IN_FEATURES)
        self.mask_coarse_side_size = m.POOLER_RESOLUTION
        self._feature_scales = {k: 1.0 / v.stride for k, v in input_shape.items()}
        in_channels = int(sum(input_shape[f].channels for f in self.mask_coarse_in_features))
        self.coarse_head = CoarseMaskHead(cfg, ShapeSpec(channels=in_channels, width=self.mask_coarse_side_size,
                                                         height=self.mask_coarse_side_size))
        self.mask_point_on = m.POINT_HEAD_ON
        if not self.mask_point_on:
            return
        p = cfg.MODEL.POINT_HEAD
        assert cfg.MODEL.ROI_HEADS.NUM_CLASSES == p.NUM_CLASSES
        self.mask_point_in_features = list(p.IN_FEATURES)
        self.mask_point_train_num_points = p.TRAIN_NUM_POINTS
        self.mask_point_oversample_ratio = p.OVERSAMPLE_RATIO
        self.mask_point_importance_sample_ratio = p.IMPORTANCE_SAMPLE_RATIO
        self.mask_point_subdivision_steps = p.SUBDIVISION_STEPS
        self.mask_point_subdivision_num_points = p.SUBDIVISION_NUM_POINTS
        self._point_channels = int(sum(input_shape[f].channels for f in self.mask_point_in_features))
        self.point_head = build_point_head(cfg, ShapeSpec(channels=self._point_channels, width=1, height=1))
        self.accuracy_stats = None      # int32 [accurate points, points] of the last training step, on the device

    # ---- the feature maps: one fan view per reader, so that their gradients meet in one map (layers/grad_fan.py)
    def _views(self, features):
        names = list(self.mask_coarse_in_features)
        if self.mask_point_on:
            names += self.mask_point_in_features
        views = {}
        for k in set(names):
            views[k] = list(grad_fan.fan_out(features[k], names.count(k)))
        return views

    def _sources(self, views, names, extra=None):
        out, col = [], 0
        for k in names:
            f = views[k].pop()
            out.append((f, PR.SHARED, self._feature_scales[k], col))
            col += int(f.shape[1])
        if extra is not None:
            out.append((extra, PR.PER_ROI, 1.0, col))
            col += int(extra.shape[1])
        return out, col

    def forward(self, features, instances, targets=None):
        views = self._views(features)
        key = "proposal_boxes" if self.training else "pred_boxes"
        boxes = cat([getattr(x, key).tensor for x in instances]) if instances else None
        counts = [len(x) for x in instances]
        num = sum(counts)
        some = next(iter(features.values()))
        roi_image = PR.roi_image_index(counts, some.device)
        coarse = self._forward_mask_coarse(views, boxes, roi_image, num, some)
        if self.training:
            from .roi_heads import cropped_mask_targets
            classes = cat([x.gt_classes for x in instances]).to(torch.int64)
            tgt = cropped_mask_targets(instances, targets, coarse.shape[-1])
            losses = {"loss_mask": mask_rcnn_loss(coarse, classes, tgt) if num else coarse.sum() * 0}
            if self.mask_point_on:
                losses["loss_mask_point"] = self._point_loss(views, coarse, instances, targets, boxes, roi_image, classes)
            return losses
        logits = self._subdivision(views, coarse, instances, boxes, roi_image) if self.mask_point_on else coarse
        classes = cat([x.pred_classes for x in instances]).to(torch.int64) if num else None
        if logits.shape[1] > 1 and num:
            logits = logits[torch.arange(num, device=logits.device), classes][:, None]
        probs = logits[:, :1].sigmoid()
        for prob, inst in zip(probs.split(counts, dim=0), instances):
            inst.pred_masks = prob                      # (Ri, 1, M, M), as mask_rcnn_inference stores them
        return instances

    def _forward_mask_coarse(self, views, boxes, roi_image, num, some):
        side = self.mask_coarse_side_size
        if num == 0:
            zero = sum(p.sum() for p in self.coarse_head.parameters()) * 0
            s = self.coarse_head.output_side_resolution
            return some.new_zeros((0, self.coarse_head.num_classes, s, s)) + zero
        src, _ = self._sources(views, self.mask_coarse_in_features)
        rows, _ = PR.point_gather(src, boxes, roi_image, grid_side=side, space_to_depth=True, want_coords=False)
        return self.coarse_head.layers_rows(rows, num)

    def _point_loss(self, views, coarse, instances, targets, boxes, roi_image, classes):
        """mask_head.py:216-237 + roi_mask_point_loss, on the row buffer."""
        num = coarse.shape[0]
        if num == 0:
            return coarse.sum() * 0 + sum(p.sum() for p in self.point_head.parameters()) * 0
        with torch.no_grad():
            point_coords = PR.get_uncertain_point_coords_with_randomness(
                coarse, PR.UncertaintyOfClasses(classes), self.mask_point_train_num_points,
                self.mask_point_oversample_ratio, self.mask_point_importance_sample_ratio)
        src, width = self._sources(views, self.mask_point_in_features, coarse)
        rows, coords = PR.point_gather(src, boxes, roi_image, point_coords)
        logits = self.point_head.forward_rows(rows, rows[:, width - coarse.shape[1]:width])
        masks = [t.gt_masks if len(t) else None for t in targets]
        matched = cat([x.matched_gt_idx for x in instances if len(x)])
        loss, stats, _ = PR.point_loss(logits, None if logits.shape[1] == 1 else classes, masks, roi_image, matched,
                                       coords, self.mask_point_train_num_points, return_details=True)
        self.accuracy_stats = stats                     # point_rend/accuracy = stats[0] / stats[1], left on the device
        return loss

    @torch.no_grad()
    def _subdivision(self, views, coarse, instances, boxes, roi_image):
        """mask_head.py:238-275 on the predicted class's channel: (R, 1, 7 * 2^steps, ...)."""
        num = coarse.shape[0]
        if num == 0:
            return coarse                               # (the reference: the subdivision cannot take an empty list)
        classes = cat([x.pred_classes for x in instances]).to(torch.int64)
        coarse = coarse.contiguous()
        m = coarse[torch.arange(num, device=coarse.device), classes][:, None].contiguous() if coarse.shape[1] > 1 \
            else coarse.clone()
        src, width = self._sources(views, self.mask_point_in_features, coarse)
        steps, n_points = self.mask_point_subdivision_steps, self.mask_point_subdivision_num_points
        for step in range(steps):
            h, w = m.shape[-2:]
            skip = n_points >= 4 * (2 * h) * (2 * w) and step < steps - 1
            m, idx, coords = PR.point_subdivide(m, 0 if skip else n_points)
            if skip:
                continue
            rows, _ = PR.point_gather(src, boxes, roi_image, coords, want_coords=False)
            logits = self.point_head.forward_rows(rows, rows[:, width - coarse.shape[1]:width])
            PR.point_scatter(m, idx, logits, classes)
        return m


@ROI_HEADS_REGISTRY.register()
class PointRendROIHeads(StandardROIHeads):
    """projects/PointRend/point_rend/roi_heads.py: StandardROIHeads that still loads checkpoints and configs written
    before the two heads moved under `mask_head` (`mask_point_head.` / `mask_coarse_head.` keys,
    `ROI_MASK_HEAD.NAME: "CoarseMaskHead"`)."""

    _version = 2

    def __init__(self, cfg, input_shape):
        if cfg.MODEL.MASK_ON and cfg.MODEL.ROI_MASK_HEAD.NAME != "PointRendMaskHead":
            logging.getLogger(__name__).warning("Config of PointRend models have changed! Applying automatic conversion now ...")
            assert cfg.MODEL.ROI_MASK_HEAD.NAME == "CoarseMaskHead"
            cfg = cfg.clone()
            cfg.defrost()
            cfg.MODEL.ROI_MASK_HEAD.NAME = "PointRendMaskHead"
            cfg.MODEL.ROI_MASK_HEAD.POOLER_TYPE = ""
        super().__init__(cfg, input_shape)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        version = local_metadata.get("version", None)
        if version is None or version < 2:
            for k in list(state_dict.keys()):
                newk = k
                if k.startswith(prefix + "mask_point_head"):
                    newk = k.replace(prefix + "mask_point_head", prefix + "mask_head.point_head")
                if k.startswith(prefix + "mask_coarse_head"):
                    newk = k.replace(prefix + "mask_coarse_head", prefix + "mask_head.coarse_head")
                if newk != k:
                    state_dict[newk] = state_dict.pop(k)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)
