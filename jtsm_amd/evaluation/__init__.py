"""Evaluation on the device.  Pascal VOC detection: AP at IoU 0.50:0.05:0.95 and CorLoc (jtsm_amd/csrc/voc_eval.hip).
Panoptic quality (PQ / SQ / RQ, all / things / stuff) and the semantic-segmentation metrics (mIoU, fwIoU, mACC, pACC)
of the JTSM model (jtsm_amd/csrc/panoptic_eval.hip).  COCO box / mask AP (AP, AP50, AP75, APs, APm, APl and per-category
AP) and keypoint AP (OKS: AP, AP50, AP75, APm, APl; jtsm_amd/csrc/coco_eval.hip).
DatasetEvaluators([SemSegEvaluator, COCOEvaluator, COCOPanopticEvaluator]) is the reference's `coco_panoptic_seg`
evaluator list (projects/WSL/tools/train_net.py:163-174); COCOEvaluator alone serves its COCO detection and keypoint
configs.  Not here: gathering results across ranks (comm.gather — evaluate one rank's images, or
concatenate before process()), proposal (AR) evaluation, LVIS, polygon rasterisation, the predictions'
JSON / PNG / RLE dumps, the reference's visualisation function and the results/VOC2007/Main/comp3_*.txt submission
files."""
from .coco_evaluation import COCOEvaluator, COCOGroundTruth, coco_accumulate, coco_image, coco_image_keypoints
from .evaluator import DatasetEvaluator, DatasetEvaluators, inference_on_dataset
from .panoptic_evaluation import COCOPanopticEvaluator, PanopticGroundTruth, pq_accumulate
from .pascal_voc_evaluation import PascalVOCDetectionEvaluator, VOCGroundTruth, voc_eval
from .sem_seg_evaluation import SemSegEvaluator, confusion_accumulate

__all__ = ["DatasetEvaluator", "DatasetEvaluators", "inference_on_dataset", "PascalVOCDetectionEvaluator",
           "VOCGroundTruth", "voc_eval", "COCOPanopticEvaluator", "PanopticGroundTruth", "pq_accumulate",
           "SemSegEvaluator", "confusion_accumulate", "COCOEvaluator", "COCOGroundTruth", "coco_image",
           "coco_image_keypoints", "coco_accumulate"]
