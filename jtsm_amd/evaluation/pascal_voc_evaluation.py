"""Pascal VOC detection evaluation on the device: PascalVOCDetectionEvaluator of the reference
(detectron2/evaluation/pascal_voc_evaluation.py — its own variant: AP at IoU 0.50:0.05:0.95 and CorLoc) without the
host round trip.  process() keeps references to the detections where the model left them; evaluate() concatenates them,
makes one library call (jtsm_voc_eval: quantise, sort, match, AP — jtsm_amd/csrc/voc_eval.hip) and reads 20 x C doubles
back once.  Semantics, and the one declared difference (equal quantised scores rank in arrival order): DESIGN.md §4e."""
import os
import xml.etree.ElementTree as ET
from collections import OrderedDict

import numpy as np
import torch

from .. import _lib as L
from .evaluator import DatasetEvaluator

NUM_THRESHOLDS = 10          # IoU 0.50 : 0.05 : 0.95; row t of the tables is (50 + 5 t) / 100


class VOCGroundTruth:
    """The annotations as the evaluator consumes them: image_ids (N, the evaluation's image list), and the objects of
    the evaluated classes sorted by (class, image), file order inside: gt_boxes (G,4) int32 as in the XML (1-based),
    gt_difficult (G,) uint8, gt_offsets (C*N+1,) int32 — the CSR over (class, image), class-major.  NumPy arrays;
    the evaluator uploads them once."""

    def __init__(self, image_ids, objects, num_classes):
        """objects: rows (image index, class, difficult, xmin, ymin, xmax, ymax) in file order."""
        self.image_ids = list(image_ids)
        self.num_images, self.num_classes = len(self.image_ids), int(num_classes)
        assert self.num_images >= 1 and self.num_classes >= 1
        assert len(set(self.image_ids)) == self.num_images, "duplicate image ids"
        o = np.asarray(objects, np.int64).reshape(-1, 7)
        assert o.size == 0 or (0 <= o[:, 0].min() and o[:, 0].max() < self.num_images
                               and 0 <= o[:, 1].min() and o[:, 1].max() < self.num_classes)
        key = o[:, 1] * self.num_images + o[:, 0]
        perm = np.argsort(key, kind="stable")
        o, key = o[perm], key[perm]
        cells = self.num_classes * self.num_images
        self.gt_offsets = np.zeros(cells + 1, np.int32)
        np.cumsum(np.bincount(key, minlength=cells), out=self.gt_offsets[1:])
        self.gt_boxes = np.ascontiguousarray(o[:, 3:7].astype(np.int32))
        self.gt_difficult = (o[:, 2] != 0).astype(np.uint8)

    @classmethod
    def from_voc_xml(cls, annotation_dir, image_set_file, class_names):
        """Annotations/<id>.xml of every id listed in ImageSets/Main/<split>.txt: per object the fields the reference's
        parse_rec uses (name, difficult, bndbox); objects of other classes are left out."""
        with open(image_set_file, "r") as f:
            image_ids = [x.strip() for x in f.readlines()]
        index = {n: i for i, n in enumerate(class_names)}
        objects = []
        for i, image_id in enumerate(image_ids):
            tree = ET.parse(os.path.join(annotation_dir, image_id + ".xml"))
            for obj in tree.findall("object"):
                c = index.get(obj.find("name").text)
                if c is None:
                    continue
                bbox = obj.find("bndbox")
                objects.append([i, c, int(obj.find("difficult").text)]
                               + [int(bbox.find(k).text) for k in ("xmin", "ymin", "xmax", "ymax")])
        return cls(image_ids, objects, len(class_names))

    @classmethod
    def from_dataset_dicts(cls, dicts, num_classes):
        """detectron2-format dicts (image_id, annotations: category_id, bbox, optional difficult, default 0).  Boxes
        are XYXY_ABS as the VOC loader makes them — xmin and ymin moved to 0-based — so 1 is added back."""
        image_ids, objects = [], []
        for i, d in enumerate(dicts):
            image_ids.append(d["image_id"])
            for a in d.get("annotations", []):
                x0, y0, x1, y1 = (int(round(float(v))) for v in a["bbox"])
                objects.append([i, int(a["category_id"]), int(a.get("difficult", 0)), x0 + 1, y0 + 1, x1, y1])
        return cls(image_ids, objects, num_classes)

    def to(self, device):
        """-> dict of device tensors (boxes, difficult, offsets)."""
        return dict(boxes=torch.from_numpy(self.gt_boxes).to(device),
                    difficult=torch.from_numpy(self.gt_difficult).to(device),
                    offsets=torch.from_numpy(self.gt_offsets).to(device))


@torch.no_grad()
def voc_eval(det_boxes, det_scores, det_classes, det_images, gt, num_images, num_classes, use_07_metric,
             with_bits=False):
    """One jtsm_voc_eval call.  det_boxes (D,4) float32, det_scores (D,) float32, det_classes / det_images (D,) int32;
    gt: VOCGroundTruth.to(device).  Nothing is read back: -> dict of device tensors, `tables` (20 C + 4 + C doubles:
    ap (10,C), corloc (10,C), stats (4), counts (C,2) int32) and views of it, plus tp_bits / fp_bits (int16 holding
    the uint16 words) and order (int32) per detection in input order when with_bits."""
    L.require_gpu(det_boxes, det_scores, det_classes, det_images, gt["boxes"], gt["difficult"], gt["offsets"])
    assert det_boxes.dtype == det_scores.dtype == torch.float32
    assert det_classes.dtype == det_images.dtype == gt["boxes"].dtype == gt["offsets"].dtype == torch.int32
    assert gt["difficult"].dtype == torch.uint8
    D, G, N, C = det_scores.numel(), gt["difficult"].numel(), int(num_images), int(num_classes)
    assert det_boxes.shape == (D, 4) and gt["offsets"].numel() == C * N + 1
    det_boxes, det_scores = det_boxes.contiguous(), det_scores.contiguous()
    det_classes, det_images = det_classes.contiguous(), det_images.contiguous()
    dev = gt["offsets"].device
    T = NUM_THRESHOLDS
    tables = torch.empty(2 * T * C + 4 + C, dtype=torch.float64, device=dev)
    out = dict(tables=tables, ap=tables[:T * C].view(T, C), corloc=tables[T * C:2 * T * C].view(T, C),
               stats=tables[2 * T * C:2 * T * C + 4], counts=tables[2 * T * C + 4:].view(torch.int32).view(C, 2))
    if with_bits:
        out["tp_bits"] = torch.empty(D, dtype=torch.int16, device=dev)
        out["fp_bits"] = torch.empty(D, dtype=torch.int16, device=dev)
        out["order"] = torch.empty(D, dtype=torch.int32, device=dev)
    nz = lambda t: L.ptr(t) if t is not None and t.numel() else None  # noqa: E731
    lib = L.lib()
    ws = torch.empty(lib.jtsm_voc_eval_workspace_bytes(D, G, C), dtype=torch.uint8, device=dev)
    L.check(lib.jtsm_voc_eval(
        nz(det_boxes), nz(det_scores), nz(det_classes), nz(det_images), D, nz(gt["boxes"]), nz(gt["difficult"]),
        L.ptr(gt["offsets"]), G, N, C, int(bool(use_07_metric)), L.ptr(out["ap"]), L.ptr(out["corloc"]),
        L.ptr(out["counts"]), L.ptr(out["stats"]), nz(out.get("tp_bits")), nz(out.get("fp_bits")),
        nz(out.get("order")), L.ptr(ws), ws.numel(), L.stream()), "voc_eval")
    return out


def split_tables(tables, num_classes):
    """The host copy of voc_eval's `tables` -> (ap (10,C), corloc (10,C), stats (4,), counts (C,2)) NumPy arrays."""
    T, C = NUM_THRESHOLDS, num_classes
    t = tables.numpy()
    return (t[:T * C].reshape(T, C), t[T * C:2 * T * C].reshape(T, C), t[2 * T * C:2 * T * C + 4],
            t[2 * T * C + 4:].view(np.int32).reshape(C, 2))


def result_dict(ap, corloc):
    """The reference's result from the (10, C) tables (pascal_voc_evaluation.py:128-168): values x100, np.mean over the
    classes per threshold, AP / CL the mean over the ten thresholds."""
    m_ap = [np.mean([v * 100 for v in row]) for row in ap]
    m_cl = [np.mean([v * 100 for v in row]) for row in corloc]
    ret = OrderedDict()
    ret["bbox"] = {"AP": np.mean(m_ap), "AP50": m_ap[0], "AP75": m_ap[5]}
    ret["bbox CorLoc"] = {"CL": np.mean(m_cl), "CL50": m_cl[0], "CL75": m_cl[5]}
    return ret


class PascalVOCDetectionEvaluator(DatasetEvaluator):
    """class_names: the evaluated classes, index = pred_classes value; ground_truth: VOCGroundTruth over the same
    classes; year: 2007 = the 11-point AP, 2012 = the area under the precision envelope.  One rank's detections only
    (the reference's comm.gather is not reproduced)."""

    def __init__(self, class_names, ground_truth, year, device="cuda"):
        assert year in (2007, 2012), year
        assert len(class_names) == ground_truth.num_classes
        self._class_names = list(class_names)
        self._is_2007 = year == 2007
        self._gt = ground_truth
        self._index = {image_id: i for i, image_id in enumerate(ground_truth.image_ids)}
        self._gt_dev = ground_truth.to(device)          # uploaded once
        self.reset()

    def reset(self):
        self._boxes, self._scores, self._classes = [], [], []      # device tensors, as the model returned them
        self._images, self._lengths = [], []                       # host: image index and detections per image

    def process(self, inputs, outputs):
        """Keeps references to pred_boxes / scores / pred_classes of outputs[i]["instances"] (no copy to the host)."""
        for inp, out in zip(inputs, outputs):
            image_id = inp["image_id"]
            if image_id not in self._index:
                raise ValueError("image_id %r is not in the ground truth's image list" % (image_id,))
            inst = out["instances"]
            boxes = inst.pred_boxes
            self._boxes.append(boxes.tensor if hasattr(boxes, "tensor") else boxes)
            self._scores.append(inst.scores)
            self._classes.append(inst.pred_classes)
            self._images.append(self._index[image_id])
            self._lengths.append(len(inst.scores))

    def evaluate(self):
        """-> {"bbox": {"AP", "AP50", "AP75"}, "bbox CorLoc": {"CL", "CL50", "CL75"}}, values x100."""
        C = len(self._class_names)
        if sum(self._lengths) == 0:
            return result_dict(np.zeros((NUM_THRESHOLDS, C)), np.zeros((NUM_THRESHOLDS, C)))
        dev = self._gt_dev["offsets"].device
        boxes = torch.cat([b.reshape(-1, 4) for b in self._boxes]).to(torch.float32)
        scores = torch.cat(self._scores).to(torch.float32)
        classes = torch.cat(self._classes).to(torch.int32)
        images = torch.repeat_interleave(torch.tensor(self._images, dtype=torch.int32),
                                         torch.tensor(self._lengths)).to(dev)
        out = voc_eval(boxes, scores, classes, images, self._gt_dev, self._gt.num_images, C, self._is_2007)
        ap, corloc, stats, counts = split_tables(out["tables"].cpu(), C)       # the one read-back
        self.last_tables = dict(ap=ap, corloc=corloc, counts=counts)
        if stats[2] != 0:
            raise ValueError("%d detections carry a class outside [0, %d)" % (int(stats[2]), C))
        if not (stats[0] >= 0.0 and stats[1] <= 1.0):
            raise ValueError("scores must lie in [0, 1] (the evaluation ranks their thousandths); got [%r, %r]"
                             % (float(stats[0]), float(stats[1])))
        bad = [self._class_names[c] for c in range(C) if np.isnan(corloc[:, c]).any()]
        if bad:
            raise ValueError("CorLoc is undefined for %s: detections, but no image with a non-difficult box "
                             "(the reference divides by zero here)" % ", ".join(bad))
        return result_dict(ap, corloc)
