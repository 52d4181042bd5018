"""Semantic segmentation metrics on the device: SemSegEvaluator of the reference
(detectron2/evaluation/sem_seg_evaluation.py) without copying every arg-max to the host.  process() runs the arg-max
entry point on the (C,H,W) logits and one jtsm_confusion_accumulate call per image (jtsm_amd/csrc/panoptic_eval.hip)
into a (C+1)^2 int64 table that stays on the device; evaluate() reads it back once and derives mIoU, fwIoU, mACC, pACC
and the per-class values in fp64 as the reference's evaluate() :124-148 does.  The JSON / RLE dump of the predictions
is not reproduced.  DESIGN.md §4f."""
from collections import OrderedDict

import numpy as np
import torch

from .. import _lib as L
from ..layers.postprocess import argmax_channels
from .evaluator import DatasetEvaluator

CONFUSION_LDS_CELLS = 16384      # kConfLdsCells of panoptic_eval.hip (jtsm_confusion_lds_cells()): (C+1)^2 counters up
#                                  to this are kept in LDS, i.e. C <= 127; global atomics above


def sem_seg_gt_from_files(paths):
    """{image_id: path of a single-channel label PNG} -> {image_id: (H,W) uint8 / int32 array}, decoded with PIL."""
    from PIL import Image

    out = {}
    for image_id, path in paths.items():
        a = np.asarray(Image.open(path))
        out[image_id] = a if a.dtype == np.uint8 else a.astype(np.int32)
    return out


@torch.no_grad()
def confusion_accumulate(pred, gt, num_classes, ignore_label, conf, force_global=False):
    """One jtsm_confusion_accumulate call.  pred (H,W) int64 and gt (H,W) uint8 or int32 on the device; conf: the
    ((C+1)^2 + 1,) int64 device tensor whose last word counts the pixels left out (pred outside [0,C), gt outside [0,C]
    after the ignore label became C).  Nothing is read back."""
    L.require_gpu(pred, gt, conf)
    C = int(num_classes)
    assert pred.dtype == torch.int64 and conf.dtype == torch.int64 and conf.numel() == (C + 1) ** 2 + 1
    assert gt.dtype in (torch.uint8, torch.int32) and pred.shape == gt.shape, (gt.dtype, pred.shape, gt.shape)
    pred, gt = pred.contiguous(), gt.contiguous()
    L.check(L.lib().jtsm_confusion_accumulate(L.ptr(pred), L.ptr(gt), gt.element_size(), pred.numel(), C,
                                              int(ignore_label), L.ptr(conf), L.ptr(conf[(C + 1) ** 2:]),
                                              int(bool(force_global)), L.stream()), "confusion_accumulate")
    return conf


def sem_seg_metrics(conf_matrix, class_names):
    """The reference's numbers from the (C+1, C+1) matrix [pred, gt], its quirks kept: accuracy AND IoU of a class are
    taken only where the class occurs in the ground truth (NaN elsewhere), while mIoU divides their sum by the number of
    classes that occur in the ground truth or the prediction."""
    C = len(class_names)
    inner = np.asarray(conf_matrix, dtype=np.int64)[:C, :C]
    correct = inner.diagonal().astype(np.float64)
    gt_pixels = inner.sum(axis=0).astype(np.float64)
    pred_pixels = inner.sum(axis=1).astype(np.float64)
    in_gt = gt_pixels > 0
    in_either = (gt_pixels + pred_pixels) > 0
    acc, iou = np.full(C, np.nan), np.full(C, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        acc[in_gt] = correct[in_gt] / gt_pixels[in_gt]
        iou[in_gt] = correct[in_gt] / (gt_pixels + pred_pixels - correct)[in_gt]
        weight = gt_pixels / np.sum(gt_pixels)
        summary = {"mIoU": np.sum(iou[in_gt]) / np.sum(in_either), "fwIoU": np.sum(iou[in_gt] * weight[in_gt]),
                   "mACC": np.sum(acc[in_gt]) / np.sum(in_gt), "pACC": np.sum(correct) / np.sum(gt_pixels)}
    res = OrderedDict()
    for key in ("mIoU", "fwIoU"):
        res[key] = 100 * summary[key]
    for name, v in zip(class_names, iou):
        res["IoU-%s" % name] = 100 * v
    for key in ("mACC", "pACC"):
        res[key] = 100 * summary[key]
    for name, v in zip(class_names, acc):
        res["ACC-%s" % name] = 100 * v
    return res


class SemSegEvaluator(DatasetEvaluator):
    """class_names: the evaluated classes, index = channel of the logits; ignore_label: the ground-truth value left out
    (it takes the matrix's extra column); ground_truth: {image_id: (H,W) uint8 or int32 label array}.  One rank's images
    only."""

    def __init__(self, class_names, ignore_label, ground_truth, device="cuda"):
        self._class_names = list(class_names)
        self._num_classes = len(self._class_names)
        self._ignore_label = int(ignore_label)
        self._gt = ground_truth
        self._device = torch.device(device)
        self.reset()

    def reset(self):
        self._conf = torch.zeros((self._num_classes + 1) ** 2 + 1, dtype=torch.int64, device=self._device)

    def process(self, inputs, outputs):
        """outputs[i]["sem_seg"]: (C,H,W) float logits on the device; inputs[i]["image_id"] names the ground truth."""
        for inp, out in zip(inputs, outputs):
            image_id = inp["image_id"]
            if image_id not in self._gt:
                raise ValueError("image_id %r is not in the ground truth" % (image_id,))
            logits = out["sem_seg"]
            if logits.shape[0] != self._num_classes:
                raise ValueError("sem_seg has %d channels, %d classes are evaluated" % (logits.shape[0], self._num_classes))
            gt = np.ascontiguousarray(self._gt[image_id])
            if gt.dtype != np.uint8:
                gt = gt.astype(np.int32)
            if tuple(logits.shape[1:]) != gt.shape:
                raise ValueError("image %r: prediction %s, ground truth %s" % (image_id, tuple(logits.shape[1:]), gt.shape))
            pred = argmax_channels(logits.to(torch.float32))
            confusion_accumulate(pred, torch.from_numpy(gt).to(self._device), self._num_classes, self._ignore_label,
                                 self._conf)

    def evaluate(self):
        """-> {"sem_seg": {mIoU, fwIoU, IoU-<class>..., mACC, pACC, ACC-<class>...}}, values x100."""
        side = self._num_classes + 1
        host = self._conf.cpu().numpy()                                                  # the one read-back
        self.last_conf_matrix = host[:side * side].reshape(side, side).copy()
        if host[side * side] != 0:
            raise ValueError("%d pixels carry a prediction outside [0, %d) or a label outside [0, %d] and %d"
                             % (int(host[side * side]), self._num_classes, self._num_classes - 1, self._ignore_label))
        return OrderedDict({"sem_seg": sem_seg_metrics(self.last_conf_matrix, self._class_names)})
