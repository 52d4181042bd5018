"""Data ABI between model components (detectron2/structures): the subset the JTSM path touches."""
from .boxes import Boxes, pairwise_iou
from .image_list import ImageList
from .instances import Instances
from .keypoints import Keypoints, heatmaps_to_keypoints
from .rotated_boxes import RotatedBoxes
from .rotated_boxes import pairwise_iou as pairwise_iou_rotated

__all__ = ["Boxes", "pairwise_iou", "ImageList", "Instances", "RotatedBoxes", "pairwise_iou_rotated",
           "Keypoints", "heatmaps_to_keypoints"]
