"""COCO box and mask AP on the device: COCOEvaluator of the reference (detectron2/evaluation/coco_evaluation.py — its
bbox and segm tasks through COCOeval_opt, evaluation/fast_eval_api.py) without the host round trip and without
pycocotools.  process() makes one library call per image and task (jtsm_coco_image: ranks, IoUs, matching —
jtsm_amd/csrc/coco_eval.hip) on the boxes and masks where inference left them and keeps one 32-byte record per
detection on the device; evaluate() concatenates the records, makes one more call (jtsm_coco_accumulate: sort,
precision / recall tables), reads the tables back once per task and summarises them with NumPy as pycocotools'
_summarize does.  Semantics: DESIGN.md §4g.

Not reproduced: the keypoints task (OKS; the model side exists), _eval_box_proposals (AR of proposals), comm.gather across ranks (one rank's images only), the
JSON / .pth dumps, LVIS, polygon rasterisation (ground-truth masks are bitmasks).  The AR lines of the summary are kept
in `last_eval[task]["stats"]`; the reference does not report them either."""
import json
from collections import OrderedDict

import numpy as np
import torch

from .. import _lib as L
from .evaluator import DatasetEvaluator

# pycocotools' Params.setDetParams, as COCOeval_opt uses them; these very doubles go to the device
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
METRICS = ["AP", "AP50", "AP75", "APs", "APm", "APl"]
NUM_THRESHOLDS, NUM_AREAS = len(IOU_THRS), len(AREA_RNG)
MAX_GT_PER_IMAGE = 4096      # jtsm_coco_image: one matched bit per 64 ground-truth rows in a lane's 64-bit word


def pack_masks(masks):
    """(G, H, W) boolean -> (G, ceil(H W / 64)) uint64: pixel p of the flat (row-major) map is bit p % 64 of word
    p / 64, the tail zero."""
    m = np.ascontiguousarray(np.asarray(masks) != 0)
    G = m.shape[0]
    pixels = int(np.prod(m.shape[1:]))
    words = (pixels + 63) // 64
    if G == 0:
        return np.zeros((0, words), dtype=np.uint64)
    flat = m.reshape(G, pixels)
    packed = np.packbits(flat, axis=1, bitorder="little")             # (the last byte's tail is zero)
    out = np.zeros((G, words * 8), dtype=np.uint8)
    out[:, :packed.shape[1]] = packed
    return out.view("<u8").reshape(G, words)


def mask_from_rle_counts(counts, height, width):
    """An uncompressed COCO RLE (`counts` a list of run lengths, column-major, starting with zeros) -> (H, W) bool."""
    runs = np.asarray(counts, dtype=np.int64)
    if runs.sum() != height * width:
        raise ValueError("RLE runs sum to %d, the image has %d pixels" % (int(runs.sum()), height * width))
    values = np.zeros(len(runs), dtype=bool)
    values[1::2] = True
    return np.repeat(values, runs).reshape(width, height).T


class COCOGroundTruth:
    """Per image id the objects of the evaluated categories, sorted by category index (annotation order inside): `cats`
    (G,) int32, `boxes` (G,4) float64 XYWH, `area` (G,) float64 — the annotation's area field —, `iscrowd` (G,) uint8,
    `cat_start` (K+1,) int32 and, if the image has masks, `words` (G, ceil(H W / 64)) uint64 with `mask_shape`.  NumPy
    arrays; the evaluator uploads an image's set when it is processed.  `image_ids` is sorted ascending: the
    accumulation order (np.unique(imgIds))."""

    def __init__(self, num_categories):
        self.num_categories = int(num_categories)
        assert self.num_categories >= 1
        self._items = {}
        self.missing_masks = {}      # image id -> description of the first annotation without a usable mask

    @property
    def image_ids(self):
        return sorted(self._items)

    def __contains__(self, image_id):
        return image_id in self._items

    def __getitem__(self, image_id):
        return self._items[image_id]

    def has_masks(self, image_id):
        it = self._items[image_id]
        return len(it["cats"]) == 0 or it["words"] is not None

    def add(self, image_id, cats, boxes, area, iscrowd, masks=None):
        assert image_id not in self._items, "duplicate image id %r" % (image_id,)
        K = self.num_categories
        cats = np.asarray(cats, dtype=np.int64).reshape(-1)
        G = len(cats)
        if G > MAX_GT_PER_IMAGE:
            raise ValueError("image %r has %d objects (at most %d)" % (image_id, G, MAX_GT_PER_IMAGE))
        assert G == 0 or (0 <= cats.min() and cats.max() < K), "category indices are 0 .. K-1"
        boxes = np.asarray(boxes, dtype=np.float64).reshape(G, 4)
        area = np.asarray(area, dtype=np.float64).reshape(G)
        iscrowd = (np.asarray(iscrowd).reshape(G) != 0).astype(np.uint8)
        perm = np.argsort(cats, kind="stable")
        cat_start = np.zeros(K + 1, np.int32)
        np.cumsum(np.bincount(cats, minlength=K), out=cat_start[1:])
        words, shape = None, None
        if masks is not None:
            masks = np.asarray(masks)
            assert masks.ndim == 3 and masks.shape[0] == G, masks.shape
            shape = tuple(masks.shape[1:])
            words = pack_masks(masks[perm])
        self._items[image_id] = dict(
            cats=cats[perm].astype(np.int32), boxes=np.ascontiguousarray(boxes[perm]),
            area=np.ascontiguousarray(area[perm]), iscrowd=np.ascontiguousarray(iscrowd[perm]), cat_start=cat_start,
            words=words, mask_shape=shape, perm=perm)

    @classmethod
    def from_arrays(cls, image_ids, cats, boxes, areas, iscrowds, num_categories, masks=None):
        """Parallel lists over the images: category indices (G,), XYWH boxes (G,4), areas (G,), iscrowd (G,), and
        optionally (G,H,W) bitmasks."""
        gt = cls(num_categories)
        for i, image_id in enumerate(image_ids):
            gt.add(image_id, cats[i], boxes[i], areas[i], iscrowds[i], None if masks is None else masks[i])
        return gt

    @classmethod
    def from_dataset_dicts(cls, dicts, num_categories):
        """detectron2-format dicts (image_id, height, width, annotations: category_id — the contiguous index —, bbox
        with bbox_mode 0 = XYXY_ABS (the default) or 1 = XYWH_ABS, iscrowd, optionally a (H,W) bitmask array under
        `segmentation` and `area`).  Without `area`: the mask's pixel count, else the box's w * h — what the reference's
        convert_to_coco_dict writes.  An image has masks only if every annotation carries a bitmask."""
        gt = cls(num_categories)
        for d in dicts:
            anns = d.get("annotations", [])
            cats, boxes, areas, crowd, masks = [], [], [], [], []
            for a in anns:
                b = [float(v) for v in a["bbox"]]
                if int(a.get("bbox_mode", 0)) == 0:
                    b = [b[0], b[1], b[2] - b[0], b[3] - b[1]]
                seg = a.get("segmentation")
                mask = np.asarray(seg) != 0 if isinstance(seg, np.ndarray) and seg.ndim == 2 else None
                if mask is None and d["image_id"] not in gt.missing_masks:
                    gt.missing_masks[d["image_id"]] = "annotation %d of image %r" % (len(cats), d["image_id"])
                cats.append(int(a["category_id"]))
                boxes.append(b)
                crowd.append(int(a.get("iscrowd", 0)))
                areas.append(float(a["area"]) if "area" in a else
                             (float(mask.sum()) if mask is not None else b[2] * b[3]))
                masks.append(mask)
            all_masks = len(masks) > 0 and all(m is not None for m in masks)
            gt.add(d["image_id"], cats, boxes, areas, crowd, np.stack(masks) if all_masks else None)
        return gt

    @classmethod
    def from_coco_json(cls, json_path, categories, mask_loader=None):
        """A COCO instances file.  categories: the dataset's category ids (or dicts with "id") in evaluation-index
        order; annotations of other categories are left out.  Boxes, area and iscrowd come from the JSON.  Masks come
        from uncompressed-RLE `counts` lists (column-major) or from mask_loader(annotation) -> (H, W) array; a polygon
        or a compressed string without a loader leaves the image without segm ground truth (`missing_masks` names the
        annotation, and a segm evaluation of that image raises)."""
        index = {(c["id"] if isinstance(c, dict) else c): i for i, c in enumerate(categories)}
        with open(json_path, "r") as f:
            data = json.load(f)
        sizes = {im["id"]: (int(im["height"]), int(im["width"])) for im in data["images"]}
        per_image = OrderedDict((im["id"], []) for im in data["images"])
        for ann in data.get("annotations", []):
            if ann["category_id"] in index:
                per_image[ann["image_id"]].append(ann)
        gt = cls(len(index))
        for image_id, anns in per_image.items():
            masks = []
            for ann in anns:
                seg, mask = ann.get("segmentation"), None
                if mask_loader is not None:
                    mask = np.asarray(mask_loader(ann)) != 0
                elif isinstance(seg, dict) and isinstance(seg.get("counts"), (list, tuple)):
                    mask = mask_from_rle_counts(seg["counts"], int(seg["size"][0]), int(seg["size"][1]))
                if mask is None:
                    gt.missing_masks.setdefault(image_id, "annotation id %r of image %r" % (ann.get("id"), image_id))
                elif mask.shape != sizes[image_id]:
                    raise ValueError("annotation id %r: mask %s, image %s" % (ann.get("id"), mask.shape, sizes[image_id]))
                masks.append(mask)
            all_masks = len(masks) > 0 and all(m is not None for m in masks)
            gt.add(image_id, [index[a["category_id"]] for a in anns], [a["bbox"] for a in anns],
                   [a["area"] for a in anns], [a.get("iscrowd", 0) for a in anns],
                   np.stack(masks) if all_masks else None)
        return gt


def new_state(num_categories, device):
    """The evaluation's constants and zeroed running totals on the device: iou_thrs (10), area_rng (4,2), rec_thrs
    (101) float64, max_dets (3) int32; npos (K,4) and stats (2) int64."""
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)  # noqa: E731
    return dict(iou_thrs=f(IOU_THRS), area_rng=f(np.array(AREA_RNG)), rec_thrs=f(REC_THRS),
                max_dets=torch.tensor(MAX_DETS, dtype=torch.int32).to(device),
                npos=torch.zeros(int(num_categories), NUM_AREAS, dtype=torch.int64, device=device),
                stats=torch.zeros(2, dtype=torch.int64, device=device))


@torch.no_grad()
def coco_image(boxes, scores, classes, masks, gt, image_index, state, with_debug=False):
    """One jtsm_coco_image call.  boxes (n,4) float32 XYXY, scores (n,) float32, classes (n,) int32, masks (n,H,W)
    bool / uint8 or None (the bbox task) — device tensors; gt: dict of device tensors boxes (G,4) float64 XYWH, area
    (G,) float64, iscrowd (G,) uint8, cat_start (K+1,) int32 and, for segm, words (G, ceil(H W / 64)) int64 holding
    the uint64 words, with mask_shape.  state: new_state().  Nothing is read back: -> dict(records (n,4) int64, and
    with_debug ious (n,G) float64 and rank (n,) int32)."""
    L.require_gpu(boxes, scores, classes, masks, gt["boxes"], gt["area"], gt["iscrowd"], gt["cat_start"],
                  gt.get("words"), state["npos"])
    assert boxes.dtype == scores.dtype == torch.float32 and classes.dtype == gt["cat_start"].dtype == torch.int32
    assert gt["boxes"].dtype == gt["area"].dtype == torch.float64 and gt["iscrowd"].dtype == torch.uint8
    n, G, K = scores.numel(), gt["area"].numel(), state["npos"].shape[0]
    assert boxes.shape == (n, 4) and gt["boxes"].shape == (G, 4) and gt["cat_start"].numel() == K + 1
    boxes, scores, classes = boxes.contiguous(), scores.contiguous(), classes.contiguous()
    segm = masks is not None
    H = W = 0
    words = None
    if segm:
        if masks.dtype == torch.bool:
            masks = masks.view(torch.uint8)
        assert masks.dtype == torch.uint8 and masks.dim() == 3 and masks.shape[0] == n, (masks.dtype, masks.shape)
        masks = masks.contiguous()
        H, W = int(masks.shape[1]), int(masks.shape[2])
        words = gt["words"]
        assert words.dtype == torch.int64 and words.is_contiguous()
        assert tuple(words.shape) == (G, (H * W + 63) // 64), (tuple(words.shape), G, H, W)
    dev = state["npos"].device
    out = dict(records=torch.empty(n, 4, dtype=torch.int64, device=dev))
    if with_debug:
        out["ious"] = torch.full((n, G), -1.0, dtype=torch.float64, device=dev)
        out["rank"] = torch.full((n,), -1, dtype=torch.int32, device=dev)
    nz = lambda t: L.ptr(t) if t is not None and t.numel() else None  # noqa: E731
    lib = L.lib()
    nbytes = lib.jtsm_coco_image_workspace_bytes(n, G, K, H, W, MAX_DETS[-1])
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    # a segm call without detections and without ground truth has nothing to tell the task by: nothing to do either
    L.check(lib.jtsm_coco_image(
        nz(boxes), nz(scores), nz(classes), nz(masks) if segm else None, n, H, W, nz(gt["boxes"]), nz(gt["area"]),
        nz(gt["iscrowd"]), L.ptr(gt["cat_start"]), nz(words) if segm else None, G, K, int(image_index), MAX_DETS[-1],
        L.ptr(state["iou_thrs"]), L.ptr(state["area_rng"]), nz(out["records"]), L.ptr(state["npos"]),
        L.ptr(state["stats"]), nz(out.get("ious")), nz(out.get("rank")), L.ptr(ws), ws.numel(), L.stream()),
        "coco_image")
    return out


@torch.no_grad()
def coco_accumulate(records, num_images, state):
    """One jtsm_coco_accumulate call over the concatenated records (D,4) int64.  -> dict of device tensors: `tables`
    (one float64 vector) and its views precision, scores (T,R,K,A,M) and recall (T,K,A,M)."""
    L.require_gpu(records, state["npos"])
    assert records.dtype == torch.int64 and records.dim() == 2 and records.shape[1] == 4
    records = records.contiguous()
    D, K = records.shape[0], state["npos"].shape[0]
    T, R, A, M = NUM_THRESHOLDS, len(REC_THRS), NUM_AREAS, len(MAX_DETS)
    dev = state["npos"].device
    big, small = T * R * K * A * M, T * K * A * M
    tables = torch.empty(2 * big + small, dtype=torch.float64, device=dev)
    out = dict(tables=tables, precision=tables[:big].view(T, R, K, A, M), scores=tables[big:2 * big].view(T, R, K, A, M),
               recall=tables[2 * big:].view(T, K, A, M))
    lib = L.lib()
    ws = torch.empty(lib.jtsm_coco_accumulate_workspace_bytes(D, K), dtype=torch.uint8, device=dev)
    L.check(lib.jtsm_coco_accumulate(
        L.ptr(records) if D else None, D, K, int(num_images), L.ptr(state["npos"]), L.ptr(state["rec_thrs"]), R,
        L.ptr(state["max_dets"]), M, L.ptr(out["precision"]), L.ptr(out["scores"]), L.ptr(out["recall"]), L.ptr(ws),
        ws.numel(), L.stream()), "coco_accumulate")
    return out


def split_tables(tables, num_categories):
    """The host copy of coco_accumulate's `tables` -> (precision, scores (T,R,K,A,M), recall (T,K,A,M)) NumPy arrays."""
    T, R, K, A, M = NUM_THRESHOLDS, len(REC_THRS), int(num_categories), NUM_AREAS, len(MAX_DETS)
    t = tables.numpy()
    big = T * R * K * A * M
    return t[:big].reshape(T, R, K, A, M), t[big:2 * big].reshape(T, R, K, A, M), t[2 * big:].reshape(T, K, A, M)


def summarize(precision, recall):
    """pycocotools' COCOeval._summarizeDets: the twelve stats — AP, AP50, AP75, APs, APm, APl at maxDets 100, then AR at
    maxDets 1 / 10 / 100 and ARs, ARm, ARl; the mean of the entries > -1, or -1 without any."""
    def one(ap, iou=None, area=0, max_det=MAX_DETS[-1]):
        m = MAX_DETS.index(max_det)
        s = precision[:, :, :, area, m] if ap else recall[:, :, area, m]
        if iou is not None:
            s = s[np.where(iou == IOU_THRS)[0]]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    return np.array([one(1), one(1, iou=.5), one(1, iou=.75), one(1, area=1), one(1, area=2), one(1, area=3),
                     one(0, max_det=MAX_DETS[0]), one(0, max_det=MAX_DETS[1]), one(0), one(0, area=1), one(0, area=2),
                     one(0, area=3)], dtype=np.float64)


def derive_coco_results(stats, precision, class_names=None):
    """The reference's _derive_coco_results (coco_evaluation.py:288-354) without its logging: values x100, NaN for a
    negative stat; with more than one class name also "AP-<name>" from precision[:, :, k, 0, -1]; stats None (no
    predictions at all): NaN for every metric."""
    if stats is None:
        return {metric: float("nan") for metric in METRICS}
    results = {metric: float(stats[idx] * 100 if stats[idx] >= 0 else "nan") for idx, metric in enumerate(METRICS)}
    if class_names is None or len(class_names) <= 1:
        return results
    assert len(class_names) == precision.shape[2]
    for idx, name in enumerate(class_names):
        p = precision[:, :, idx, 0, -1]
        p = p[p > -1]
        results["AP-" + "{}".format(name)] = float((np.mean(p) if p.size else float("nan")) * 100)
    return results


class COCOEvaluator(DatasetEvaluator):
    """ground_truth: COCOGroundTruth; class_names: the evaluated categories in index order (index = pred_classes
    value) for the per-category AP; tasks: a subset of ("bbox", "segm"), or None to infer it from the first processed
    output as the reference does (bbox, plus segm when pred_masks is present).  All images of the ground truth count
    (the reference's default imgIds), processed or not."""

    def __init__(self, ground_truth, class_names=None, tasks=None, device="cuda"):
        assert class_names is None or len(class_names) == ground_truth.num_categories
        assert tasks is None or (len(tasks) and set(tasks) <= {"bbox", "segm"}), tasks
        self._gt = ground_truth
        self._class_names = None if class_names is None else list(class_names)
        self._given_tasks = None if tasks is None else tuple(tasks)
        self._device = torch.device(device)
        self._index = {image_id: i for i, image_id in enumerate(ground_truth.image_ids)}    # ascending image id
        self.reset()

    def reset(self):
        self._tasks = self._given_tasks
        self._state, self._records, self._seen, self._padded = {}, {"bbox": [], "segm": []}, set(), set()
        self._num_predictions = 0
        self.last_eval = {}

    def _state_of(self, task):
        if task not in self._state:
            self._state[task] = new_state(self._gt.num_categories, self._device)
        return self._state[task]

    def _upload(self, image_id, segm):
        it = self._gt[image_id]
        up = lambda a: torch.from_numpy(a).to(self._device)  # noqa: E731
        gt = dict(boxes=up(it["boxes"]), area=up(it["area"]), iscrowd=up(it["iscrowd"]), cat_start=up(it["cat_start"]))
        if segm:
            if not self._gt.has_masks(image_id):
                raise ValueError("segm evaluation needs ground-truth masks: %s has none"
                                 % self._gt.missing_masks.get(image_id, "image %r" % (image_id,)))
            gt["mask_shape"] = it["mask_shape"]
            if it["words"] is not None:
                gt["words"] = up(it["words"].view(np.int64))
        return gt

    def process(self, inputs, outputs):
        """outputs[i]["instances"]: pred_boxes (Boxes or (n,4) tensor, XYXY), scores, pred_classes (contiguous category
        indices) and optionally pred_masks (n,H,W) bool at the ground truth's resolution, on the device."""
        for inp, out in zip(inputs, outputs):
            if "instances" not in out:
                continue
            image_id = inp["image_id"]
            if image_id not in self._index:
                raise ValueError("image_id %r is not in the ground truth" % (image_id,))
            if image_id in self._seen:
                raise ValueError("image_id %r was processed twice" % (image_id,))
            inst = out["instances"]
            if self._tasks is None:
                self._tasks = ("bbox", "segm") if inst.has("pred_masks") else ("bbox",)
            boxes = inst.pred_boxes
            boxes = (boxes.tensor if hasattr(boxes, "tensor") else boxes).reshape(-1, 4).to(torch.float32)
            scores, classes = inst.scores.to(torch.float32), inst.pred_classes.to(torch.int32)
            n = scores.numel()
            for task in self._tasks:
                if task == "segm" and not inst.has("pred_masks"):
                    raise ValueError("segm evaluation needs pred_masks (image %r)" % (image_id,))
                segm = task == "segm" and n > 0       # (without detections only npos is touched: no masks needed)
                gt = self._upload(image_id, segm)
                masks = None
                if segm:
                    masks = inst.pred_masks
                    if "words" not in gt:             # an image without ground truth
                        gt["words"] = torch.zeros(0, (masks.shape[1] * masks.shape[2] + 63) // 64, dtype=torch.int64,
                                                  device=self._device)
                    elif tuple(masks.shape[1:]) != tuple(gt["mask_shape"]):
                        raise ValueError("image %r: predicted masks %s, ground truth %s"
                                         % (image_id, tuple(masks.shape[1:]), tuple(gt["mask_shape"])))
                self._records[task].append(coco_image(boxes, scores, classes, masks, gt, self._index[image_id],
                                                      self._state_of(task))["records"])
            self._seen.add(image_id)
            self._num_predictions += n

    def _add_unprocessed(self, task):
        """The ground truth of the images that were never processed counts in npos: one call without detections each."""
        state = self._state_of(task)
        empty = dict(b=torch.zeros(0, 4, dtype=torch.float32, device=self._device),
                     s=torch.zeros(0, dtype=torch.float32, device=self._device),
                     c=torch.zeros(0, dtype=torch.int32, device=self._device))
        for image_id, i in self._index.items():
            if image_id in self._seen or len(self._gt[image_id]["cats"]) == 0:
                continue
            gt = self._upload(image_id, False)                     # (only areas and crowd flags matter)
            coco_image(empty["b"], empty["s"], empty["c"], None, gt, i, state)

    def evaluate(self):
        """-> {"bbox": {AP, AP50, AP75, APs, APm, APl[, AP-<name> ...]}, "segm": {...}}, values x100 (NaN where a
        metric has no entry, and for every metric when there was no prediction at all).  `last_eval[task]` holds
        precision, scores, recall, npos and the twelve summary stats."""
        results = OrderedDict()
        tasks = self._tasks if self._tasks is not None else ("bbox",)
        K = self._gt.num_categories
        for task in tasks:
            if self._num_predictions == 0:
                results[task] = derive_coco_results(None, None)
                continue
            if task not in self._padded:                      # (a second evaluate() must not count them again)
                self._add_unprocessed(task)
                self._padded.add(task)
            state = self._state_of(task)
            records = torch.cat(self._records[task])
            out = coco_accumulate(records, max(len(self._index), 1), state)
            host = torch.cat([out["tables"], state["npos"].reshape(-1).view(torch.float64),
                              state["stats"].view(torch.float64)]).cpu()                    # the one read-back
            big = out["tables"].numel()
            precision, scores, recall = split_tables(host[:big], K)
            npos = host[big:big + K * NUM_AREAS].numpy().view(np.int64).reshape(K, NUM_AREAS)
            bad = int(host[big + K * NUM_AREAS:].numpy().view(np.int64)[0])
            if bad:
                raise ValueError("%d detections carry a class outside [0, %d)" % (bad, K))
            stats = summarize(precision, recall)
            self.last_eval[task] = dict(precision=precision, scores=scores, recall=recall, npos=npos, stats=stats)
            results[task] = derive_coco_results(stats, precision, self._class_names)
        return results
