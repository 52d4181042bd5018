"""COCO box, mask and keypoint AP on the device: COCOEvaluator of the reference (detectron2/evaluation/coco_evaluation.py
— its bbox, segm and keypoints tasks through COCOeval_opt, evaluation/fast_eval_api.py) without the host round trip and
without pycocotools.  process() makes one library call per image and task (jtsm_coco_image / jtsm_coco_image_keypoints:
ranks, IoUs or OKS, matching — jtsm_amd/csrc/coco_eval.hip) on the boxes, masks and keypoints where inference left them
and keeps one 32-byte record per detection on the device; evaluate() concatenates the records, makes one more call
(jtsm_coco_accumulate: sort, precision / recall tables), reads the tables back once per task and summarises them with
NumPy as pycocotools' _summarize does.  Semantics: DESIGN.md §4g.

Not reproduced: keypoints under test-time augmentation, _eval_box_proposals (AR of proposals), comm.gather across ranks
(one rank's images only), the JSON / .pth dumps, LVIS, polygon rasterisation (ground-truth masks are bitmasks).  The AR
lines of the summary are kept in `last_eval[task]["stats"]`; the reference does not report them either."""
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
# pycocotools' Params.setKpParams: the thresholds above, one maxDets entry, no "small" range
KP_MAX_DETS = [20]
KP_AREA_RNG = [[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
KP_METRICS = ["AP", "AP50", "AP75", "APm", "APl"]
KP_NUM_AREAS = len(KP_AREA_RNG)
COCO_KPT_OKS_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89,
                                .89]) / 10.0
MAX_KEYPOINTS = 64           # jtsm_coco_image_keypoints


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
    `cat_start` (K+1,) int32 and, if the image has masks, `words` (G, ceil(H W / 64)) uint64 with `mask_shape`; if it
    has keypoints, `keypoints` (G,P,3) float64 (x, y, v as the COCO JSON holds them) and `num_keypoints` (G,) int64.
    NumPy arrays; the evaluator uploads an image's set when it is processed.  `image_ids` is sorted ascending: the
    accumulation order (np.unique(imgIds))."""

    def __init__(self, num_categories):
        self.num_categories = int(num_categories)
        assert self.num_categories >= 1
        self._items = {}
        self.missing_masks = {}      # image id -> description of the first annotation without a usable mask
        self.missing_keypoints = {}  # image id -> description of the first annotation without keypoints

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

    def has_keypoints(self, image_id):
        it = self._items[image_id]
        return len(it["cats"]) == 0 or it["keypoints"] is not None

    def add(self, image_id, cats, boxes, area, iscrowd, masks=None, keypoints=None, num_keypoints=None):
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
        if keypoints is not None and G > 0:
            keypoints = np.asarray(keypoints, dtype=np.float64).reshape(G, -1, 3)
            if num_keypoints is None:
                num_keypoints = (keypoints[:, :, 2] > 0).sum(1)
            num_keypoints = np.asarray(num_keypoints, dtype=np.int64).reshape(G)
            keypoints, num_keypoints = np.ascontiguousarray(keypoints[perm]), np.ascontiguousarray(num_keypoints[perm])
        else:                                   # (an image without objects needs none)
            keypoints = num_keypoints = None
        self._items[image_id] = dict(
            cats=cats[perm].astype(np.int32), boxes=np.ascontiguousarray(boxes[perm]),
            area=np.ascontiguousarray(area[perm]), iscrowd=np.ascontiguousarray(iscrowd[perm]), cat_start=cat_start,
            words=words, mask_shape=shape, keypoints=keypoints, num_keypoints=num_keypoints, perm=perm)

    @classmethod
    def from_arrays(cls, image_ids, cats, boxes, areas, iscrowds, num_categories, masks=None, keypoints=None,
                    num_keypoints=None):
        """Parallel lists over the images: category indices (G,), XYWH boxes (G,4), areas (G,), iscrowd (G,), and
        optionally (G,H,W) bitmasks, (G,P,3) keypoints and (G,) num_keypoints (default: the count of v > 0)."""
        gt = cls(num_categories)
        at = lambda seq, i: None if seq is None else seq[i]  # noqa: E731
        for i, image_id in enumerate(image_ids):
            gt.add(image_id, cats[i], boxes[i], areas[i], iscrowds[i], at(masks, i), at(keypoints, i),
                   at(num_keypoints, i))
        return gt

    @classmethod
    def from_dataset_dicts(cls, dicts, num_categories):
        """detectron2-format dicts (image_id, height, width, annotations: category_id — the contiguous index —, bbox
        with bbox_mode 0 = XYXY_ABS (the default) or 1 = XYWH_ABS, iscrowd, optionally a (H,W) bitmask array under
        `segmentation` and `area`).  Without `area`: the mask's pixel count, else the box's w * h — what the reference's
        convert_to_coco_dict writes.  An image has masks only if every annotation carries a bitmask.  `keypoints`
        (3 P values or (P,3)): x and y minus 0.5 as convert_to_coco_dict writes them (datasets/coco.py:361-373; the
        annotation is left alone), `num_keypoints` from the field or else the count of v > 0; an image has keypoints
        only if every annotation carries them."""
        gt = cls(num_categories)
        for d in dicts:
            anns = d.get("annotations", [])
            cats, boxes, areas, crowd, masks, kps, nkp = [], [], [], [], [], [], []
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
                kp = a.get("keypoints")
                if kp is None:
                    gt.missing_keypoints.setdefault(d["image_id"], "annotation %d of image %r"
                                                    % (len(cats) - 1, d["image_id"]))
                else:
                    kp = np.array(kp, dtype=np.float64).reshape(-1, 3)
                    kp[:, :2] -= 0.5
                    nkp.append(int(a["num_keypoints"]) if "num_keypoints" in a else int((kp[:, 2] > 0).sum()))
                kps.append(kp)
            all_masks = len(masks) > 0 and all(m is not None for m in masks)
            all_kps = len(kps) > 0 and all(k is not None for k in kps)
            gt.add(d["image_id"], cats, boxes, areas, crowd, np.stack(masks) if all_masks else None,
                   _stack_keypoints(kps, d["image_id"]) if all_kps else None, nkp if all_kps else None)
        return gt

    @classmethod
    def from_coco_json(cls, json_path, categories, mask_loader=None):
        """A COCO instances file.  categories: the dataset's category ids (or dicts with "id") in evaluation-index
        order; annotations of other categories are left out.  Boxes, area and iscrowd come from the JSON.  Masks come
        from uncompressed-RLE `counts` lists (column-major) or from mask_loader(annotation) -> (H, W) array; a polygon
        or a compressed string without a loader leaves the image without segm ground truth (`missing_masks` names the
        annotation, and a segm evaluation of that image raises).  `keypoints` and `num_keypoints` are read as they
        stand; an image whose annotations do not all carry keypoints has no keypoint ground truth
        (`missing_keypoints` names the annotation)."""
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
            kps = [np.asarray(a["keypoints"], np.float64).reshape(-1, 3) if "keypoints" in a else None for a in anns]
            for ann, kp in zip(anns, kps):
                if kp is None:
                    gt.missing_keypoints.setdefault(image_id, "annotation id %r of image %r" % (ann.get("id"), image_id))
            all_kps = len(kps) > 0 and all(k is not None for k in kps)
            nkp = [int(a["num_keypoints"]) if "num_keypoints" in a else int((k[:, 2] > 0).sum())
                   for a, k in zip(anns, kps)] if all_kps else None
            gt.add(image_id, [index[a["category_id"]] for a in anns], [a["bbox"] for a in anns],
                   [a["area"] for a in anns], [a.get("iscrowd", 0) for a in anns],
                   np.stack(masks) if all_masks else None, _stack_keypoints(kps, image_id) if all_kps else None, nkp)
        return gt


def _stack_keypoints(kps, image_id):
    if len({k.shape for k in kps}) != 1:
        raise ValueError("image %r: objects with %s keypoints" % (image_id, sorted({k.shape[0] for k in kps})))
    return np.stack(kps)


def new_state(num_categories, device, keypoints=False):
    """The evaluation's constants and zeroed running totals on the device: iou_thrs (10), area_rng (4,2), rec_thrs
    (101) float64, max_dets (3) int32; npos (K,4) and stats (2) int64.  keypoints: max_dets (1) = [20] and the three
    area ranges of the task; the device's records keep four, so the last row is repeated and its column of npos and
    of the tables is dropped on the host."""
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)  # noqa: E731
    area_rng = KP_AREA_RNG + KP_AREA_RNG[-1:] if keypoints else AREA_RNG
    return dict(iou_thrs=f(IOU_THRS), area_rng=f(np.array(area_rng)), rec_thrs=f(REC_THRS),
                max_dets=torch.tensor(KP_MAX_DETS if keypoints else MAX_DETS, dtype=torch.int32).to(device),
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
def coco_image_keypoints(boxes, scores, classes, keypoints, gt, sigmas, image_index, state, with_debug=False):
    """One jtsm_coco_image_keypoints call.  boxes, scores, classes as coco_image; keypoints (n,P,3) float32 as the model
    leaves them (read only: the 0.5 shift happens in the kernel); gt: coco_image's boxes, area, iscrowd, cat_start plus
    keypoints (G,P,3) float64 and ignore (G,) uint8; sigmas (P,) float64 on the device; state: new_state(keypoints=True).
    -> dict(records (n,4) int64, and with_debug ious (n,G) float64 — the OKS — and rank (n,) int32)."""
    L.require_gpu(boxes, scores, classes, keypoints, gt["boxes"], gt["area"], gt["iscrowd"], gt["ignore"],
                  gt["keypoints"], gt["cat_start"], sigmas, state["npos"])
    assert boxes.dtype == scores.dtype == keypoints.dtype == torch.float32
    assert classes.dtype == gt["cat_start"].dtype == torch.int32
    assert gt["boxes"].dtype == gt["area"].dtype == gt["keypoints"].dtype == sigmas.dtype == torch.float64
    assert gt["iscrowd"].dtype == gt["ignore"].dtype == torch.uint8
    n, G, K, P = scores.numel(), gt["area"].numel(), state["npos"].shape[0], sigmas.numel()
    assert boxes.shape == (n, 4) and gt["boxes"].shape == (G, 4) and gt["cat_start"].numel() == K + 1
    assert tuple(keypoints.shape) == (n, P, 3) and tuple(gt["keypoints"].shape) == (G, P, 3), (
        tuple(keypoints.shape), tuple(gt["keypoints"].shape), P)
    assert gt["iscrowd"].numel() == gt["ignore"].numel() == G and state["max_dets"].numel() == len(KP_MAX_DETS)
    boxes, scores, classes, keypoints = boxes.contiguous(), scores.contiguous(), classes.contiguous(), keypoints.contiguous()
    gkp, sigmas = gt["keypoints"].contiguous(), sigmas.contiguous()
    dev = state["npos"].device
    out = dict(records=torch.empty(n, 4, dtype=torch.int64, device=dev))
    if with_debug:
        out["ious"] = torch.full((n, G), -1.0, dtype=torch.float64, device=dev)
        out["rank"] = torch.full((n,), -1, dtype=torch.int32, device=dev)
    nz = lambda t: L.ptr(t) if t is not None and t.numel() else None  # noqa: E731
    lib = L.lib()
    nbytes = lib.jtsm_coco_image_keypoints_workspace_bytes(n, G, K, P, KP_MAX_DETS[-1])
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    L.check(lib.jtsm_coco_image_keypoints(
        nz(boxes), nz(scores), nz(classes), nz(keypoints), n, P, nz(gt["boxes"]), nz(gt["area"]), nz(gt["iscrowd"]),
        nz(gt["ignore"]), nz(gkp), L.ptr(gt["cat_start"]), G, K, L.ptr(sigmas), int(image_index), KP_MAX_DETS[-1],
        L.ptr(state["iou_thrs"]), L.ptr(state["area_rng"]), nz(out["records"]), L.ptr(state["npos"]),
        L.ptr(state["stats"]), nz(out.get("ious")), nz(out.get("rank")), L.ptr(ws), ws.numel(), L.stream()),
        "coco_image_keypoints")
    return out


@torch.no_grad()
def coco_accumulate(records, num_images, state):
    """One jtsm_coco_accumulate call over the concatenated records (D,4) int64.  -> dict of device tensors: `tables`
    (one float64 vector) and its views precision, scores (T,R,K,A,M) and recall (T,K,A,M); M = the state's max_dets."""
    L.require_gpu(records, state["npos"])
    assert records.dtype == torch.int64 and records.dim() == 2 and records.shape[1] == 4
    records = records.contiguous()
    D, K = records.shape[0], state["npos"].shape[0]
    T, R, A, M = NUM_THRESHOLDS, len(REC_THRS), NUM_AREAS, state["max_dets"].numel()
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


def split_tables(tables, num_categories, num_max_dets=len(MAX_DETS)):
    """The host copy of coco_accumulate's `tables` -> (precision, scores (T,R,K,A,M), recall (T,K,A,M)) NumPy arrays."""
    T, R, K, A, M = NUM_THRESHOLDS, len(REC_THRS), int(num_categories), NUM_AREAS, int(num_max_dets)
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


def summarize_keypoints(precision, recall):
    """pycocotools' COCOeval._summarizeKps on the keypoints task's tables ((T,R,K,3,1) and (T,K,3,1)): the ten stats —
    AP, AP50, AP75, APm, APl, then AR, AR50, AR75, ARm, ARl — all at maxDets 20."""
    def one(ap, iou=None, area=0):
        s = precision[:, :, :, area, 0] if ap else recall[:, :, area, 0]
        if iou is not None:
            s = s[np.where(iou == IOU_THRS)[0]]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    return np.array([one(ap, **kw) for ap in (1, 0)
                     for kw in ({}, dict(iou=.5), dict(iou=.75), dict(area=1), dict(area=2))], dtype=np.float64)


def derive_coco_results(stats, precision, class_names=None, metrics=METRICS):
    """The reference's _derive_coco_results (coco_evaluation.py:288-354) without its logging: values x100, NaN for a
    negative stat; with more than one class name also "AP-<name>" from precision[:, :, k, 0, -1]; stats None (no
    predictions at all): NaN for every metric.  metrics: METRICS, or KP_METRICS for the keypoints task."""
    if stats is None:
        return {metric: float("nan") for metric in metrics}
    results = {metric: float(stats[idx] * 100 if stats[idx] >= 0 else "nan") for idx, metric in enumerate(metrics)}
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
    value) for the per-category AP; tasks: a subset of ("bbox", "segm", "keypoints"), or None to infer it from the
    first processed output as the reference does (bbox, plus segm when pred_masks is present, plus keypoints when
    pred_keypoints is present).  kpt_oks_sigmas: the OKS sigmas, one per keypoint (TEST.KEYPOINT_OKS_SIGMAS); empty:
    the 17 of COCO.  All images of the ground truth count (the reference's default imgIds), processed or not."""

    def __init__(self, ground_truth, class_names=None, tasks=None, device="cuda", kpt_oks_sigmas=()):
        assert class_names is None or len(class_names) == ground_truth.num_categories
        assert tasks is None or (len(tasks) and set(tasks) <= {"bbox", "segm", "keypoints"}), tasks
        self._gt = ground_truth
        sigmas = np.asarray(kpt_oks_sigmas, dtype=np.float64).reshape(-1)
        self._sigmas = sigmas if sigmas.size else COCO_KPT_OKS_SIGMAS
        self._dev_sigmas = None
        self._class_names = None if class_names is None else list(class_names)
        self._given_tasks = None if tasks is None else tuple(tasks)
        self._device = torch.device(device)
        self._index = {image_id: i for i, image_id in enumerate(ground_truth.image_ids)}    # ascending image id
        self.reset()

    def reset(self):
        self._tasks = self._given_tasks
        self._state, self._seen, self._padded = {}, set(), set()
        self._records = {"bbox": [], "segm": [], "keypoints": []}
        self._num_predictions = 0
        self.last_eval = {}

    def _state_of(self, task):
        if task not in self._state:
            self._state[task] = new_state(self._gt.num_categories, self._device, keypoints=task == "keypoints")
        return self._state[task]

    def _upload_keypoints(self, image_id, pred_keypoints):
        """The image's ground truth for the keypoints task; the numbers of sigmas, predicted and ground-truth keypoints
        must agree (the reference asserts it, coco_evaluation.py:561-570)."""
        if not self._gt.has_keypoints(image_id):
            raise ValueError("keypoints evaluation needs ground-truth keypoints: %s has none"
                             % self._gt.missing_keypoints.get(image_id, "image %r" % (image_id,)))
        it = self._gt[image_id]
        P, G = len(self._sigmas), len(it["cats"])
        if P > MAX_KEYPOINTS:
            raise ValueError("%d keypoint sigmas (at most %d)" % (P, MAX_KEYPOINTS))
        counts = dict(sigmas=P)
        if pred_keypoints is not None:
            counts["predictions"] = int(pred_keypoints.shape[1])
        if it["keypoints"] is not None:
            counts["ground truth"] = int(it["keypoints"].shape[1])
        if len(set(counts.values())) != 1:
            raise ValueError("image %r: the numbers of keypoints differ: %s" % (
                image_id, ", ".join("%s %d" % kv for kv in counts.items())))
        gt = self._upload(image_id, False)
        kp = it["keypoints"] if it["keypoints"] is not None else np.zeros((0, P, 3))
        nk = it["num_keypoints"] if it["num_keypoints"] is not None else np.zeros(0, np.int64)
        gt["keypoints"] = torch.from_numpy(kp).to(self._device)
        gt["ignore"] = torch.from_numpy(((it["iscrowd"] != 0) | (nk == 0)).astype(np.uint8)).to(self._device)
        assert gt["ignore"].numel() == G
        if self._dev_sigmas is None:
            self._dev_sigmas = torch.from_numpy(self._sigmas).to(self._device)
        return gt

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
        indices) and optionally pred_masks (n,H,W) bool at the ground truth's resolution and pred_keypoints (n,P,3)
        float32 (x, y, score), on the device.  Nothing of the Instances is written."""
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
                self._tasks = ("bbox",) + (("segm",) if inst.has("pred_masks") else ()) + \
                    (("keypoints",) if inst.has("pred_keypoints") else ())
            boxes = inst.pred_boxes
            boxes = (boxes.tensor if hasattr(boxes, "tensor") else boxes).reshape(-1, 4).to(torch.float32)
            scores, classes = inst.scores.to(torch.float32), inst.pred_classes.to(torch.int32)
            n = scores.numel()
            for task in self._tasks:
                if task == "keypoints":
                    if not inst.has("pred_keypoints"):
                        raise ValueError("keypoints evaluation needs pred_keypoints (image %r)" % (image_id,))
                    kp = inst.pred_keypoints.to(torch.float32)
                    if kp.dim() != 3 or kp.shape[0] != n or kp.shape[2] != 3:
                        raise ValueError("image %r: pred_keypoints of shape %s" % (image_id, tuple(kp.shape)))
                    gt = self._upload_keypoints(image_id, kp)
                    self._records[task].append(coco_image_keypoints(
                        boxes, scores, classes, kp, gt, self._dev_sigmas, self._index[image_id],
                        self._state_of(task))["records"])
                    continue
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
            if task == "keypoints":                                # (only areas and ignore flags matter)
                gt = self._upload_keypoints(image_id, None)
                P = len(self._sigmas)
                coco_image_keypoints(empty["b"], empty["s"], empty["c"],
                                     torch.zeros(0, P, 3, dtype=torch.float32, device=self._device), gt,
                                     self._dev_sigmas, i, state)
                continue
            gt = self._upload(image_id, False)                     # (only areas and crowd flags matter)
            coco_image(empty["b"], empty["s"], empty["c"], None, gt, i, state)

    def evaluate(self):
        """-> {"bbox": {AP, AP50, AP75, APs, APm, APl[, AP-<name> ...]}, "segm": {...}, "keypoints": {AP, AP50, AP75,
        APm, APl[, AP-<name> ...]}}, values x100 (NaN where a metric has no entry, and for every metric when there was
        no prediction at all).  `last_eval[task]` holds precision, scores, recall, npos and the summary stats: twelve,
        or for keypoints ten, with three area ranges and one maxDets entry in the tables."""
        results = OrderedDict()
        tasks = self._tasks if self._tasks is not None else ("bbox",)
        K = self._gt.num_categories
        for task in tasks:
            kpts = task == "keypoints"
            if self._num_predictions == 0:
                results[task] = derive_coco_results(None, None, metrics=KP_METRICS if kpts else METRICS)
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
            precision, scores, recall = split_tables(host[:big], K, len(KP_MAX_DETS if kpts else MAX_DETS))
            npos = host[big:big + K * NUM_AREAS].numpy().view(np.int64).reshape(K, NUM_AREAS)
            bad = int(host[big + K * NUM_AREAS:].numpy().view(np.int64)[0])
            if bad:
                raise ValueError("%d detections carry a class outside [0, %d)" % (bad, K))
            if kpts:                                          # the spare fourth area range of the device's records
                precision, scores = precision[:, :, :, :KP_NUM_AREAS], scores[:, :, :, :KP_NUM_AREAS]
                recall, npos = recall[:, :, :KP_NUM_AREAS], npos[:, :KP_NUM_AREAS]
            stats = summarize_keypoints(precision, recall) if kpts else summarize(precision, recall)
            self.last_eval[task] = dict(precision=precision, scores=scores, recall=recall, npos=npos, stats=stats)
            results[task] = derive_coco_results(stats, precision, self._class_names, KP_METRICS if kpts else METRICS)
        return results
