"""GeneralizedRCNNWSL — projects/WSL/wsl/modeling/meta_arch/rcnn.py:24-266: backbone -> ROI heads on precomputed
proposals, for the weakly supervised detectors (ContextLocNet here).  Training returns the loss dict (:94-159);
inference returns [{"instances": ...}] through detector_postprocess (:161-236, _postprocess :254-266), or with
do_postprocess=False the raw (results, all_scores, all_boxes).  Images go through the same uint8 -> channels-last launch
as GeneralizedMCNNWSL.preprocess_image.  Proposal generators and the CPG heads (CSC / WSJDS) are not implemented."""
import torch
from torch import nn

from ...layers.conv import planes_clear, set_segment
from ..backbone import build_backbone
from ..roi_heads import build_roi_heads
from .build import META_ARCH_REGISTRY
from .mcnn import GeneralizedMCNNWSL


@META_ARCH_REGISTRY.register()
class GeneralizedRCNNWSL(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        name = cfg.MODEL.ROI_HEADS.NAME
        if "CSC" in name or "WSJDS" in name:
            raise NotImplementedError("GeneralizedRCNNWSL: the CPG heads (%s) are not implemented" % name)
        if cfg.MODEL.PROPOSAL_GENERATOR.NAME != "PrecomputedProposals":
            raise NotImplementedError("GeneralizedRCNNWSL trains on precomputed proposals only")
        self.backbone = build_backbone(cfg)
        self.proposal_generator = None
        self.roi_heads = build_roi_heads(cfg, self.backbone.output_shape())
        assert len(cfg.MODEL.PIXEL_MEAN) == len(cfg.MODEL.PIXEL_STD)
        self.register_buffer("pixel_mean", torch.Tensor(cfg.MODEL.PIXEL_MEAN).view(-1, 1, 1))
        self.register_buffer("pixel_std", torch.Tensor(cfg.MODEL.PIXEL_STD).view(-1, 1, 1))
        self.input_format = cfg.INPUT.FORMAT

    @property
    def device(self):
        return self.pixel_mean.device

    preprocess_image = GeneralizedMCNNWSL.preprocess_image
    _pixel_stats = GeneralizedMCNNWSL._pixel_stats

    def forward(self, batched_inputs):
        if not self.training:
            return self.inference(batched_inputs)
        planes_clear()
        images = self.preprocess_image(batched_inputs)
        gt_instances = [x["instances"].to(self.device) for x in batched_inputs]
        set_segment("backbone")
        features = self.backbone(images.tensor)
        set_segment("heads")
        proposals = [x["proposals"].to(self.device) for x in batched_inputs]
        _, detector_losses = self.roi_heads(images, features, proposals, gt_instances)
        return dict(detector_losses)

    @torch.no_grad()
    def inference(self, batched_inputs, detected_instances=None, do_postprocess=True):
        assert not self.training
        if detected_instances is not None:
            raise NotImplementedError("GeneralizedRCNNWSL.inference with given boxes")
        planes_clear()
        images = self.preprocess_image(batched_inputs)
        features = self.backbone(images.tensor)
        proposals = [x["proposals"].to(self.device) for x in batched_inputs]
        results, _, all_scores, all_boxes = self.roi_heads(images, features, proposals, None)
        if do_postprocess:
            return GeneralizedMCNNWSL._postprocess(results, batched_inputs, images.image_sizes)
        return results, all_scores, all_boxes
