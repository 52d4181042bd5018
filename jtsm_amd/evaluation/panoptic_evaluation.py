"""Panoptic quality on the device: COCOPanopticEvaluator of the reference (detectron2/evaluation/
panoptic_evaluation.py — PNG files handed to panopticapi's pq_compute) without the host round trip.  process() uploads
the image's ground truth and makes one library call per image (jtsm_pq_accumulate: pair histogram, matching, totals —
jtsm_amd/csrc/panoptic_eval.hip) on the panoptic map and segment table where inference left them; evaluate() reads
4 C + 4 totals back once and averages them on the host in fp64.  Semantics and the declared differences (summation
order, counted areas, errors as stats + ValueError, NaN for an empty group): DESIGN.md §4f."""
import json
import os
from collections import OrderedDict

import numpy as np
import torch

from .. import _lib as L
from .evaluator import DatasetEvaluator

PQ_LDS_CELLS = 16384      # kPqLdsCells of panoptic_eval.hip (jtsm_pq_lds_cells()): the pair histogram of an image
#                           with (G+1)(P+1) <= this is built in LDS, a larger one with global atomics


class PanopticGroundTruth:
    """Per image id a dense (H,W) int32 segment map (0 = VOID, r + 1 = row r) and the (G,2) int32 table {evaluation
    category in [0,C), iscrowd} in annotation order.  NumPy arrays; the evaluator uploads an image's pair when it is
    processed."""

    def __init__(self):
        self._items = OrderedDict()

    @property
    def image_ids(self):
        return list(self._items)

    def __contains__(self, image_id):
        return image_id in self._items

    def __getitem__(self, image_id):
        return self._items[image_id]

    def add(self, image_id, seg_map, table):
        seg_map = np.ascontiguousarray(seg_map, dtype=np.int32)
        table = np.ascontiguousarray(np.asarray(table, dtype=np.int32).reshape(-1, 2))
        assert seg_map.ndim == 2 and image_id not in self._items
        assert seg_map.size == 0 or (0 <= seg_map.min() and seg_map.max() <= len(table)), "map values are 0 .. G"
        self._items[image_id] = (seg_map, table)

    @classmethod
    def from_arrays(cls, image_ids, maps, tables):
        gt = cls()
        for image_id, m, t in zip(image_ids, maps, tables):
            gt.add(image_id, m, t)
        return gt

    @classmethod
    def from_coco_panoptic(cls, json_path, png_root, categories):
        """COCO panoptic annotations.  categories: the dataset's category ids (or dicts with "id") in evaluation-index
        order.  Every annotation's PNG is decoded with PIL (id = R + 256 G + 65536 B) and its ids are renumbered to
        row + 1 in segments_info order; a pixel id that segments_info does not list becomes VOID (the reference skips
        such labels).  Areas are counted from the map by the evaluation; the JSON's `area` fields are ignored."""
        from PIL import Image

        index = {(c["id"] if isinstance(c, dict) else c): i for i, c in enumerate(categories)}
        with open(json_path, "r") as f:
            data = json.load(f)
        gt = cls()
        for ann in data["annotations"]:
            rgb = np.asarray(Image.open(os.path.join(png_root, ann["file_name"])).convert("RGB"), dtype=np.int64)
            ids = rgb[..., 0] + 256 * rgb[..., 1] + 65536 * rgb[..., 2]
            seg_ids = np.array([s["id"] for s in ann["segments_info"]], dtype=np.int64)
            table = []
            for s in ann["segments_info"]:
                if s["category_id"] not in index:
                    raise ValueError("image %r: segment %r has the unknown category %r"
                                     % (ann["image_id"], s["id"], s["category_id"]))
                table.append([index[s["category_id"]], int(s.get("iscrowd", 0))])
            dense = np.zeros(ids.shape, np.int32)
            if len(seg_ids):
                order = np.argsort(seg_ids, kind="stable")
                pos = np.clip(np.searchsorted(seg_ids[order], ids), 0, len(seg_ids) - 1)
                hit = seg_ids[order][pos] == ids
                dense[hit] = (order[pos][hit] + 1).astype(np.int32)
            gt.add(ann["image_id"], dense, table)
        return gt


def new_totals(num_categories, device):
    """Zeroed running totals on the device: `tables` (4 C + 4 int64 words) and views of it: tp, fp, fn (C) int64,
    iou_sum (C) float64, stats (4) int64."""
    C = int(num_categories)
    t = torch.zeros(4 * C + 4, dtype=torch.int64, device=device)
    return dict(tables=t, tp=t[:C], fp=t[C:2 * C], fn=t[2 * C:3 * C], iou_sum=t[3 * C:4 * C].view(torch.float64),
                stats=t[4 * C:])


def split_totals(tables, num_categories):
    """The host copy of `tables` -> (tp, fp, fn (C,) int64, iou_sum (C,) float64, stats (4,) int64) NumPy arrays."""
    C = int(num_categories)
    t = tables.numpy()
    return t[:C], t[C:2 * C], t[2 * C:3 * C], t[3 * C:4 * C].view(np.float64), t[4 * C:]


@torch.no_grad()
def pq_accumulate(pred, pred_table, num_pred, thing_cat, stuff_cat, gt, gt_table, totals, force_global=False):
    """One jtsm_pq_accumulate call: one image added into `totals` (new_totals).  pred / gt (H,W) int32 maps, pred_table
    (P,5) int32, num_pred (1,) int32 on the device, thing_cat / stuff_cat int32, gt_table (G,2) int32 — all device
    tensors.  Nothing is read back."""
    L.require_gpu(pred, pred_table, num_pred, thing_cat, stuff_cat, gt, gt_table, totals["tables"])
    for t in (pred, pred_table, num_pred, thing_cat, stuff_cat, gt, gt_table):
        assert t.dtype == torch.int32, t.dtype
    assert pred.shape == gt.shape, (pred.shape, gt.shape)
    pred, gt = pred.contiguous(), gt.contiguous()
    assert pred_table.dim() == 2 and pred_table.shape[1] == 5 and gt_table.dim() == 2 and gt_table.shape[1] == 2
    pred_table, gt_table = pred_table.contiguous(), gt_table.contiguous()
    thing_cat, stuff_cat = thing_cat.contiguous(), stuff_cat.contiguous()
    P, G, C = pred_table.shape[0], gt_table.shape[0], totals["tp"].numel()
    nz = lambda t: L.ptr(t) if t.numel() else None  # noqa: E731
    lib = L.lib()
    nbytes = lib.jtsm_pq_accumulate_workspace_bytes(G, P, C)
    if nbytes == 0:
        raise ValueError("pq_accumulate: a pair table of (%d+1) x (%d+1) counters is too large" % (G, P))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
    L.check(lib.jtsm_pq_accumulate(
        nz(pred), nz(pred_table), L.ptr(num_pred), P, nz(thing_cat), thing_cat.numel(), nz(stuff_cat),
        stuff_cat.numel(), nz(gt), nz(gt_table), G, pred.numel(), C, L.ptr(totals["tp"]), L.ptr(totals["fp"]),
        L.ptr(totals["fn"]), L.ptr(totals["iou_sum"]), L.ptr(totals["stats"]), int(bool(force_global)), L.ptr(ws),
        ws.numel(), L.stream()), "pq_accumulate")
    return totals


def pq_average(tp, fp, fn, iou_sum, categories_isthing):
    """panopticapi's pq_average over All / Things / Stuff in fp64 on the host: per category with tp + fp + fn > 0,
    pq = iou / (tp + fp/2 + fn/2), sq = iou / tp (0 when tp = 0), rq = tp / (tp + fp/2 + fn/2); plain means over the
    counted categories, `n` of them; NaN for a group with none (the package divides by zero)."""
    out = OrderedDict()
    for name, want in (("All", None), ("Things", True), ("Stuff", False)):
        pq, sq, rq, n = 0.0, 0.0, 0.0, 0
        for c, isthing in enumerate(categories_isthing):
            if want is not None and bool(isthing) != want:
                continue
            t, p, f, iou = int(tp[c]), int(fp[c]), int(fn[c]), float(iou_sum[c])
            if t + p + f == 0:
                continue
            denom = t + 0.5 * p + 0.5 * f
            n += 1
            pq += iou / denom
            sq += iou / t if t != 0 else 0
            rq += t / denom
        nan = float("nan")
        out[name] = {"pq": pq / n if n else nan, "sq": sq / n if n else nan, "rq": rq / n if n else nan, "n": n}
    return out


class COCOPanopticEvaluator(DatasetEvaluator):
    """ground_truth: PanopticGroundTruth; thing_cat / stuff_cat: contiguous thing / stuff id of the model ->
    evaluation category index in [0, C) or -1; categories_isthing: (C,) booleans.  One rank's images only (the
    reference's comm.gather is not reproduced); the predictions.json / PNG dump is not written."""

    def __init__(self, ground_truth, thing_cat, stuff_cat, categories_isthing, device="cuda"):
        self._gt = ground_truth
        self._isthing = [bool(v) for v in categories_isthing]
        self._device = torch.device(device)
        self._thing_cat = torch.tensor(list(thing_cat), dtype=torch.int32).to(self._device)       # uploaded once
        self._stuff_cat = torch.tensor(list(stuff_cat), dtype=torch.int32).to(self._device)
        self.reset()

    def reset(self):
        self._totals = new_totals(len(self._isthing), self._device)

    def _table_of(self, segments_info):
        """The (n,5) int32 device table: the one the model left (the `table` attribute of
        combine_semantic_and_instance_outputs' list), else built from the dicts and
        uploaded (no copy to the host either way)."""
        table = getattr(segments_info, "table", None)
        if table is not None:
            return table.to(torch.int32)
        rows = [[int(s["id"]), int(bool(s["isthing"])), int(s["category_id"]), int(s.get("instance_id", -1)),
                 int(s.get("area", 0))] for s in segments_info]
        return torch.tensor(rows, dtype=torch.int32).reshape(len(rows), 5).to(self._device)

    def process(self, inputs, outputs):
        """outputs[i]["panoptic_seg"] = (panoptic (H,W) int32 on the device, segments_info) as the models' inference
        returns it; inputs[i]["image_id"] names the ground truth."""
        for inp, out in zip(inputs, outputs):
            image_id = inp["image_id"]
            if image_id not in self._gt:
                raise ValueError("image_id %r is not in the ground truth" % (image_id,))
            pan, info = out["panoptic_seg"]
            if info is None:
                raise ValueError("panoptic_seg without segments_info (the label_divisor form) is not supported")
            seg_map, gt_table = self._gt[image_id]
            if tuple(pan.shape) != seg_map.shape:
                raise ValueError("image %r: prediction %s, ground truth %s" % (image_id, tuple(pan.shape), seg_map.shape))
            table = self._table_of(info)
            num_pred = torch.full((1,), table.shape[0], dtype=torch.int32, device=self._device)
            pq_accumulate(pan.to(torch.int32), table, num_pred, self._thing_cat, self._stuff_cat,
                          torch.from_numpy(seg_map).to(self._device), torch.from_numpy(gt_table).to(self._device),
                          self._totals)

    def evaluate(self):
        """-> {"panoptic_seg": {PQ, SQ, RQ, PQ_th, SQ_th, RQ_th, PQ_st, SQ_st, RQ_st}}, values x100."""
        C = len(self._isthing)
        tp, fp, fn, iou_sum, stats = split_totals(self._totals["tables"].cpu(), C)       # the one read-back
        self.last_totals = dict(tp=tp.copy(), fp=fp.copy(), fn=fn.copy(), iou_sum=iou_sum.copy(), stats=stats.copy())
        if stats[0] or stats[1] or stats[2]:
            raise ValueError("panoptic evaluation: %d pixels carry an id that no segment row lists, %d predicted rows "
                             "have no pixel, %d rows have no evaluation category (the reference raises on each)"
                             % (int(stats[0]), int(stats[1]), int(stats[2])))
        avg = self.last_average = pq_average(tp, fp, fn, iou_sum, self._isthing)
        res = {}
        for suffix, group in (("", "All"), ("_th", "Things"), ("_st", "Stuff")):
            for m in ("pq", "sq", "rq"):
                res[m.upper() + suffix] = 100 * avg[group][m]
        return OrderedDict({"panoptic_seg": res})
