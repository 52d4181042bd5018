from .box_head import ROI_BOX_HEAD_REGISTRY, DiscriminativeAdaptionNeck, FastRCNNConvFCHead, build_box_head
from .fast_rcnn import FastRCNNOutputLayers
from .fast_rcnn_oicr import OICROutputLayers
from .fast_rcnn_tsm import TSMOutputLayers
from .mask_head import (ROI_MASK_HEAD_REGISTRY, MaskRCNNConvUpsampleHead, MaskRCNNConvUpsampleWSLHead, build_mask_head,
                        mask_rcnn_loss)
from .roi_heads import (ROI_HEADS_REGISTRY, ROIHeads, StandardROIHeads, build_roi_heads, select_foreground_proposals,
                        select_proposals_with_visible_keypoints)
from .point_head import POINT_HEAD_REGISTRY, StandardPointHead, build_point_head
from .point_rend_mask_head import CoarseMaskHead, PointRendMaskHead, PointRendROIHeads
from .roi_heads_jtsm import JTSMROIHeads
from .roi_heads_contextlocnet import ContextLocNetROIHeads
from .fast_rcnn_wsddn import WSDDNOutputLayers
from .roi_heads_cmil import CMILROIHeads
from .roi_heads_oicr import OICRROIHeads
from .roi_heads_pcl import PCLROIHeads
from .rotated_fast_rcnn import RotatedFastRCNNOutputLayers, RROIHeads, fast_rcnn_inference_rotated

_KEYPOINT_NAMES = ("ROI_KEYPOINT_HEAD_REGISTRY", "BaseKeypointRCNNHead", "KRCNNConvDeconvUpsampleHead",
                   "build_keypoint_head", "keypoint_rcnn_inference", "keypoint_rcnn_loss")


def __getattr__(name):
    """The keypoint head's names, loaded on first use: a model without keypoints never imports keypoint_head.py."""
    if name in _KEYPOINT_NAMES:
        from . import keypoint_head
        return getattr(keypoint_head, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
