"""Evaluation of the detectors.  Pascal VOC detection only: AP at IoU 0.50:0.05:0.95 and CorLoc on the device
(jtsm_amd/csrc/voc_eval.hip).  Not here: gathering detections across ranks (comm.gather — evaluate one rank's
detections, or concatenate before process()), COCO and panoptic evaluation, the reference's visualisation function and
the results/VOC2007/Main/comp3_*.txt submission files."""
from .evaluator import DatasetEvaluator, inference_on_dataset
from .pascal_voc_evaluation import PascalVOCDetectionEvaluator, VOCGroundTruth, voc_eval

__all__ = ["DatasetEvaluator", "inference_on_dataset", "PascalVOCDetectionEvaluator", "VOCGroundTruth", "voc_eval"]
