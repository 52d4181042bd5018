"""Operator layer of the MI355X JTSM hot path: the names model code imports from
``detectron2.layers`` / ``wsl.layers`` (detectron2/layers/__init__.py:1-13,
projects/WSL/wsl/layers/__init__.py:1-11) that lie on the path."""
from .cmil import ROILabel, ROIMerge, roi_label, roi_merge
from .deform_conv import DeformConv, ModulatedDeformConv, deform_conv, modulated_deform_conv
from .mist import mine_top_p
from .moi_pool import MOIPool, moi_pool
from .nms import batched_nms, batched_nms_rotated, nms_rotated
from .panoptic_deeplab import (center_loss, find_instance_center, get_instance_segmentation, get_panoptic_segmentation,
                               group_pixels, merge_semantic_and_instance, offset_loss, panoptic_deeplab_postprocess)
from .point_rend import (calculate_uncertainty, generate_regular_grid_point_coords, get_point_coords_wrt_image,
                         get_uncertain_point_coords_on_grid, get_uncertain_point_coords_with_randomness, point_sample,
                         point_sample_fine_grained_features, roi_mask_point_loss)
from .roi_align import ROIAlign, roi_align
from .roi_align_rotated import ROIAlignRotated, roi_align_rotated
from .roi_loop_pool import ROILoopPool, roi_loop_pool
from .roi_pool import ROIPool, roi_pool
from .rotated_boxes import pairwise_iou_rotated

__all__ = [k for k in globals().keys() if not k.startswith("_")]
