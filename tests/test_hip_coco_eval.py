"""GPU suite (pytest -m gpu): the device-side COCO box / mask AP evaluator (jtsm_amd/csrc/coco_eval.hip,
jtsm_amd/evaluation/coco_evaluation.py) against tests/coco_eval_ref.py, the NumPy / Python restatement of DESIGN.md
§4g, and against what the reference's compiled cocoeval.cpp recorded (tests/golden/coco_eval_reference.npz).

Bit for bit, no tolerance anywhere: the ranks; the IoU of every same-category (kept detection, ground truth) pair as
fp64 bit patterns; the matched / ignore words of every record; npos; the precision / scores / recall tables as fp64
bit patterns, and with them the result dictionary.  Shapes are the smallest at which each loop can go wrong: 64 is the
match kernel's ground-truth chunk, 100 the per-(image, category) cut, 256 (PR_CHUNK) the records per step of the
precision / recall walk and the threads of the mask-IoU workgroup."""
import ctypes

import numpy as np
import pytest
import torch

import coco_eval_ref as CR
from conftest import load_cases

pytestmark = pytest.mark.gpu

PR_CHUNK = 256
RECORD = np.dtype([("cat", "<i4"), ("image", "<i4"), ("rank", "<i4"), ("score", "<f4"), ("matched", "<u8"),
                   ("ignore", "<u8")])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want):
    return list(got) == list(want) and all(_bits([got[k]])[0] == _bits([want[k]])[0] for k in want)


def _ground_truth(dataset, K, masks):
    from jtsm_amd.evaluation import COCOGroundTruth

    return COCOGroundTruth.from_arrays(
        [im["image_id"] for im in dataset], [im["gt_cats"] for im in dataset], [im["gt_boxes"] for im in dataset],
        [im["gt_area"] for im in dataset], [im["gt_crowd"] for im in dataset], K,
        [im["gt_masks"] for im in dataset] if masks else None)


def _instances(image, cuda, masks):
    from jtsm_amd.structures import Boxes, Instances

    size = tuple(image["det_masks"].shape[1:]) if image["det_masks"] is not None else (480, 640)
    inst = Instances(size, pred_boxes=Boxes(torch.from_numpy(np.asarray(image["det_boxes"], np.float32).reshape(-1, 4)).to(cuda)),
                     scores=torch.from_numpy(np.asarray(image["det_scores"], np.float32)).to(cuda),
                     pred_classes=torch.from_numpy(np.asarray(image["det_classes"], np.int64)).to(cuda))
    if masks:
        inst.set("pred_masks", torch.from_numpy(np.asarray(image["det_masks"], bool)).to(cuda))
    return inst


def _check(cuda, dataset, K, tasks=("bbox",), class_names=None, kernels=True):
    """The evaluator end to end against the restatement (tables, npos, result dict) and, with `kernels`, every image
    through coco_image with its debug outputs (ranks, IoUs, record words).  -> (device results, restatement tables)."""
    from jtsm_amd.evaluation import COCOEvaluator
    from jtsm_amd.evaluation import coco_evaluation as CE

    masks = "segm" in tasks
    gt = _ground_truth(dataset, K, masks)
    want, tables = CR.evaluate(dataset, K, tasks, class_names)
    ev = COCOEvaluator(gt, class_names=class_names, tasks=None if tasks == ("bbox", "segm") else tasks, device=cuda)
    ev.reset()
    for im in dataset:
        ev.process([{"image_id": im["image_id"]}], [{"instances": _instances(im, cuda, masks)}])
    got = ev.evaluate()
    assert list(got) == list(want)
    for task in tasks:
        assert list(got[task]) == list(want[task])
        for k in want[task]:
            assert _bits([got[task][k]])[0] == _bits([want[task][k]])[0], (task, k, got[task][k], want[task][k])
        if not any(len(im["det_scores"]) for im in dataset):
            continue
        last = ev.last_eval[task]
        assert np.array_equal(last["npos"], tables[task]["npos"]), task
        for key in ("precision", "scores", "recall"):
            assert np.array_equal(_bits(last[key]), _bits(tables[task][key])), (task, key)
        assert np.array_equal(_bits(last["stats"]), _bits(tables[task]["stats"])), task
    if not kernels:
        return got, tables
    index = {image_id: i for i, image_id in enumerate(gt.image_ids)}
    for task in tasks:
        segm = task == "segm"
        tab = tables[task]
        state = CE.new_state(K, cuda)
        for j, im in enumerate(dataset):
            i = index[im["image_id"]]
            assert tab["order"][i] == j
            item = gt[im["image_id"]]
            up = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
            g = dict(boxes=up(item["boxes"]), area=up(item["area"]), iscrowd=up(item["iscrowd"]),
                     cat_start=up(item["cat_start"]))
            inst = _instances(im, cuda, segm)
            n = len(im["det_scores"])
            if segm:
                H, W = im["det_masks"].shape[1:]
                g["words"] = up(np.ascontiguousarray(item["words"]).view(np.int64)) if item["words"] is not None \
                    else torch.zeros(0, (H * W + 63) // 64, dtype=torch.int64, device=cuda)
                if n == 0 and len(item["cats"]) == 0:
                    continue
            out = CE.coco_image(inst.pred_boxes.tensor, inst.scores, inst.pred_classes.to(torch.int32),
                                inst.pred_masks if segm else None, g, i, state, with_debug=True)
            info = tab["per_image"][i]
            assert np.array_equal(out["rank"].cpu().numpy(), info["rank"]), (task, j)
            rec = out["records"].cpu().numpy().view(RECORD).reshape(-1)
            ious = out["ious"].cpu().numpy()
            where = np.empty(len(item["perm"]), np.int64)          # annotation row -> row of the category-sorted arrays
            where[item["perm"]] = np.arange(len(item["perm"]))
            kept = info["rank"] >= 0
            assert np.array_equal(rec["cat"], np.where(kept, np.asarray(im["det_classes"]), K))
            assert np.array_equal(rec["rank"], np.where(kept, info["rank"], 0)) and (rec["image"] == i).all()
            assert np.array_equal(rec["score"], np.asarray(im["det_scores"], np.float32))
            same = np.zeros(ious.shape, bool)
            for c in range(K):
                rows, cols = info["det_rows"][c], where[info["gt_rows"][c]] if info["gt_rows"][c] else []
                if rows and len(cols):
                    w = np.array(info["ious"][c], np.float64).reshape(len(rows), len(cols))
                    assert np.array_equal(_bits(ious[np.ix_(rows, cols)]), _bits(w)), (task, j, c)
                    same[np.ix_(rows, cols)] = True
                m, ig = CR.match_bits(tab["evals"], i, c, len(rows))
                assert rec["matched"][rows].tolist() == m and rec["ignore"][rows].tolist() == ig, (task, j, c)
            assert (ious[~same] == -1.0).all()
            assert (rec["matched"][~kept] == 0).all() and (rec["ignore"][~kept] == 0).all()
    return got, tables


def _boxes_dataset(rng, counts, gts_per_image=3, K=1, size=300.0, ties=True):
    """counts[i][c] detections of category c in image i, around gts_per_image ground-truth boxes per category."""
    dataset = []
    for i, per_cat in enumerate(counts):
        gt_cats, gt_boxes, gt_crowd, boxes, scores, classes = [], [], [], [], [], []
        for c, n in enumerate(per_cat):
            mine = []
            for _ in range(gts_per_image):
                side = [rng.uniform(8, 30), rng.uniform(34, 90), rng.uniform(97, 140)][int(rng.integers(3))]
                b = [rng.uniform(0, size - side), rng.uniform(0, size - side), side, side * rng.uniform(0.8, 1.2)]
                mine.append(b)
                gt_cats.append(c)
                gt_boxes.append(b)
                gt_crowd.append(int(rng.random() < 0.1))
            for _ in range(n):
                b = mine[int(rng.integers(len(mine)))]
                j = rng.normal(0, 0.1, 4) * np.array([b[2], b[3], b[2], b[3]])
                boxes.append([b[0] + j[0], b[1] + j[1], b[0] + j[0] + max(b[2] + j[2], 1), b[1] + j[1] + max(b[3] + j[3], 1)])
                classes.append(c)
                scores.append(rng.integers(1, 50) / 50.0 if ties else rng.random())
        p = rng.permutation(len(boxes))
        gb = np.array(gt_boxes, np.float64).reshape(-1, 4)
        dataset.append(dict(image_id=100 - 3 * i, det_boxes=np.array(boxes, np.float32).reshape(-1, 4)[p],
                            det_scores=np.array(scores, np.float32)[p], det_classes=np.array(classes, np.int64)[p],
                            det_masks=None, gt_cats=np.array(gt_cats, np.int64), gt_boxes=gb,
                            gt_area=gb[:, 2] * gb[:, 3] if len(gb) else np.zeros(0), gt_crowd=np.array(gt_crowd, np.uint8),
                            gt_masks=None))
    return dataset


# ------------------------------------------------------------------------------------------------ recorded cases
CASES = load_cases("coco_eval_reference.npz")


@pytest.mark.parametrize("name", sorted(CASES))
def test_recorded_cases_match_the_compiled_reference_and_the_restatement(cuda, name):
    f = CASES[name]
    dataset = CR.dataset_from_fields(f)
    tasks = ("bbox", "segm") if "mask_hw" in f else ("bbox",)
    names = ["c%d" % c for c in range(6)]
    got, tables = _check(cuda, dataset, 6, tasks, class_names=names)
    for task in tasks:                  # the restatement's tables are the recorded ones (tests/test_coco_eval_ref.py) —
        for key in ("precision", "scores", "recall"):     # checked here again so that this file stands on the fixture
            assert np.array_equal(_bits(tables[task][key]), _bits(f["%s_%s" % (task, key)]))
        assert np.isnan(got[task]["AP-c3"]) and got[task]["AP"] > 0


# ---------------------------------------------------------------------------------------------------- loop edges
@pytest.mark.parametrize("G", [0, 1, 64, 65, 130])
def test_ground_truth_of_one_category_around_the_chunk_of_64(cuda, G):
    """One image, one category with G ground-truth boxes — small, medium and large, every seventh a crowd — and 40
    detections; a second category keeps the CSR honest."""
    rng = np.random.default_rng(G)
    gb = [[float(rng.uniform(0, 500)), float(rng.uniform(0, 400)), s, s * float(rng.uniform(0.7, 1.3))]
          for s in rng.choice([20.0, 60.0, 110.0], G)]
    boxes, scores = [], []
    for k in range(40):
        b = gb[int(rng.integers(G))] if G and k % 4 else [50.0, 50.0, 40.0, 40.0]
        j = rng.normal(0, 0.07, 4) * np.array([b[2], b[3], b[2], b[3]])
        boxes.append([b[0] + j[0], b[1] + j[1], b[0] + j[0] + b[2] + j[2], b[1] + j[1] + b[3] + j[3]])
        scores.append(rng.integers(1, 30) / 30.0)
    if G >= 2:                                  # identical boxes at both ends of the list: the last maximum wins
        gb[0] = list(gb[-1])
    gb2 = np.array(gb + [[10.0, 10.0, 50.0, 50.0]], np.float64).reshape(-1, 4)
    image = dict(image_id=7, det_boxes=np.array(boxes + [[10, 10, 58, 61]], np.float32),
                 det_scores=np.array(scores + [0.5], np.float32), det_classes=np.array([0] * 40 + [1], np.int64),
                 det_masks=None, gt_cats=np.array([0] * G + [1], np.int64), gt_boxes=gb2, gt_area=gb2[:, 2] * gb2[:, 3],
                 gt_crowd=np.array([int(g % 7 == 6) for g in range(G)] + [0], np.uint8), gt_masks=None)
    _check(cuda, [image], 2)


@pytest.mark.parametrize("n", [99, 100, 101])
def test_detections_of_one_category_around_the_cut_at_100(cuda, n):
    rng = np.random.default_rng(n)
    dataset = _boxes_dataset(rng, [[n, 5], [3, n + 20]], K=2)
    got, tables = _check(cuda, dataset, 2)
    kept = sum(int((info["rank"] >= 0).sum()) for info in tables["bbox"]["per_image"])
    assert kept == min(n, 100) + 5 + 3 + 100


def test_ranked_detections_of_a_category_around_the_chunk_of_the_walk(cuda):
    """Categories with 0, 1, 255, 256, 257 and 600 ranked detections over seven images (at most 100 of a category in an
    image): no chunk, one partial chunk, PR_CHUNK - 1, PR_CHUNK, PR_CHUNK + 1 (the carry) and three chunks."""
    want = [0, 1, PR_CHUNK - 1, PR_CHUNK, PR_CHUNK + 1, 600]
    counts = [[0] * 6 for _ in range(7)]
    for c, total in enumerate(want):
        for i in range(7):
            counts[i][c] = min(100, total - sum(counts[k][c] for k in range(i)))
    rng = np.random.default_rng(5)
    dataset = _boxes_dataset(rng, counts, gts_per_image=2, K=6)
    assert [sum(row[c] for row in counts) for c in range(6)] == want
    got, tables = _check(cuda, dataset, 6, class_names=list("abcdef"), kernels=False)
    assert got["bbox"]["AP-a"] == 0.0 and got["bbox"]["AP-f"] > 0


def test_maxdets_1_and_10_skip_records_inside_the_walk(cuda):
    """Ranks 0, 1-9 and 10+ interleave in the score order, so the maxDets 1 / 10 walks skip records between the ones
    they count; scores without ties make the order unique."""
    rng = np.random.default_rng(11)
    dataset = _boxes_dataset(rng, [[30], [25], [40], [0], [12]], gts_per_image=4, ties=False)
    _, tables = _check(cuda, dataset, 1)
    r = tables["bbox"]["recall"]
    assert (r[:, 0, 0, 0] <= r[:, 0, 0, 1]).all() and (r[:, 0, 0, 1] <= r[:, 0, 0, 2]).all() and r[0, 0, 0, 0] < r[0, 0, 0, 2]


# --------------------------------------------------------------------------------------------------------- masks
def _mask_dataset(rng, H, W, n_images=2, K=2):
    yy, xx = np.mgrid[0:H, 0:W]
    rect = lambda x, y, w, h: (xx >= x) & (xx < x + w) & (yy >= y) & (yy < y + h)  # noqa: E731
    dataset = []
    for i in range(n_images):
        gt_boxes, gt_cats, gmasks, boxes, classes, scores, dmasks = [], [], [], [], [], [], []
        for g in range(4):
            w, h = int(rng.integers(4, W // 2)), int(rng.integers(4, H // 2))
            x, y = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
            gt_boxes.append([x, y, w, h])
            gt_cats.append(g % K)
            gmasks.append(rect(x, y, w, h))
            for _ in range(3):
                dx, dy = int(rng.integers(-3, 4)), int(rng.integers(-3, 4))
                boxes.append([x + dx, y + dy, x + dx + w, y + dy + h])
                classes.append(g % K)
                scores.append(rng.integers(1, 10) / 10.0)
                dmasks.append(rect(x + dx, y + dy, w, h))
        boxes.append([0, 0, 3, 3])                                   # an empty predicted mask
        classes.append(0)
        scores.append(0.95)
        dmasks.append(np.zeros((H, W), bool))
        boxes.append([W - 2, H - 2, W, H])                           # the last pixels: the tail of the last word
        classes.append(1)
        scores.append(0.35)
        dmasks.append(rect(W - 2, H - 2, 2, 2))
        gm = np.stack(gmasks)
        dataset.append(dict(image_id=5 - i, det_boxes=np.array(boxes, np.float32), det_scores=np.array(scores, np.float32),
                            det_classes=np.array(classes, np.int64), det_masks=np.stack(dmasks),
                            gt_cats=np.array(gt_cats, np.int64), gt_boxes=np.array(gt_boxes, np.float64),
                            gt_area=gm.reshape(len(gm), -1).sum(1).astype(np.float64),
                            gt_crowd=np.array([0, 0, 0, int(i == 0)], np.uint8), gt_masks=gm))
    return dataset


@pytest.mark.parametrize("H,W", [(37, 53), (64, 64), (127, 130)])
def test_masks_of_ragged_and_aligned_sizes(cuda, H, W):
    """37 x 53 = 1961 pixels: 31 words with a tail of 41 bits; 64 x 64: 64 whole words; 127 x 130 = 16510 pixels: 258
    words, more than the 256 threads of the mask-IoU workgroup and more than one pass of the packing grid.  Empty
    predicted masks and empty intersections are in every image."""
    dataset = _mask_dataset(np.random.default_rng(H), H, W)
    _, tables = _check(cuda, dataset, 2, ("bbox", "segm"))
    flat = [v for info in tables["segm"]["per_image"] for rows in info["ious"].values() for row in rows for v in row]
    assert 0.0 in flat and max(flat) > 0.5


def test_iou_exactly_at_a_threshold(cuda):
    """IoU 1/2 and 3/4 are IOU_THRS[0] and IOU_THRS[5] exactly: `>=` matches there and at no higher threshold."""
    assert CR.IOU_THRS[0] == 0.5 and CR.IOU_THRS[5] == 0.75
    H, W = 8, 16
    dm = np.zeros((2, H, W), bool)
    dm[0, 0, :4] = True                      # 4 pixels over a ground truth of 3 of them: 3/4
    dm[1, 2, :8] = True                      # 8 pixels over a ground truth of 4 of them: 1/2
    gm = np.zeros((2, H, W), bool)
    gm[0, 0, :3] = True
    gm[1, 2, :4] = True
    image = dict(image_id=1, det_boxes=np.array([[0, 0, 4, 1], [0, 2, 20, 12]], np.float32),
                 det_scores=np.array([0.9, 0.8], np.float32), det_classes=np.array([0, 0], np.int64), det_masks=dm,
                 gt_cats=np.array([0, 0], np.int64), gt_boxes=np.array([[0, 0, 3, 1], [0, 2, 10, 10]], np.float64),
                 gt_area=np.array([3.0, 100.0]), gt_crowd=np.zeros(2, np.uint8), gt_masks=gm)
    _, tables = _check(cuda, [image], 1, ("bbox", "segm"))
    for task in ("bbox", "segm"):
        ious = tables[task]["per_image"][0]["ious"][0]
        assert ious[0][0] == 0.75 and ious[1][1] == 0.5, (task, ious)
        m = np.array(tables[task]["evals"][(0, 0, 0)]["matches"])
        assert m[:, 0].tolist() == [1] * 6 + [0] * 4 and m[:, 1].tolist() == [2] + [0] * 9


def test_all_ground_truth_of_a_category_ignored(cuda):
    """Category 0: crowd regions only (npos = 0: its cells stay -1 although it has detections); category 1: ordinary."""
    rng = np.random.default_rng(3)
    dataset = _boxes_dataset(rng, [[6, 4], [5, 3]], K=2)
    for im in dataset:
        im["gt_crowd"] = (im["gt_cats"] == 0).astype(np.uint8)
    got, tables = _check(cuda, dataset, 2, class_names=["crowd", "plain"])
    assert (tables["bbox"]["precision"][:, :, 0] == -1).all() and np.isnan(got["bbox"]["AP-crowd"])


def test_images_without_detections_without_ground_truth_and_unprocessed(cuda):
    from jtsm_amd.evaluation import COCOEvaluator

    rng = np.random.default_rng(8)
    dataset = _boxes_dataset(rng, [[5, 2], [0, 0], [4, 4], [3, 1]], K=2)
    for key in ("gt_cats", "gt_boxes", "gt_area", "gt_crowd"):
        dataset[2][key] = dataset[2][key][:0]                               # image 2: detections, no ground truth
    _check(cuda, dataset, 2)
    # image 3 never processed: its ground truth still counts (the reference's imgIds default to every image)
    gt = _ground_truth(dataset, 2, False)
    ev = COCOEvaluator(gt, device=cuda)
    for im in dataset[:3]:
        ev.process([{"image_id": im["image_id"]}], [{"instances": _instances(im, cuda, False)}])
    got = ev.evaluate()
    left_out = dict(dataset[3], det_boxes=dataset[3]["det_boxes"][:0], det_scores=dataset[3]["det_scores"][:0],
                    det_classes=dataset[3]["det_classes"][:0])
    want, tables = CR.evaluate(dataset[:3] + [left_out], 2)
    assert np.array_equal(ev.last_eval["bbox"]["npos"], tables["bbox"]["npos"])
    assert np.array_equal(_bits(ev.last_eval["bbox"]["precision"]), _bits(tables["bbox"]["precision"]))
    assert _same(got["bbox"], want["bbox"]) and _same(ev.evaluate()["bbox"], want["bbox"])      # (twice: the same)


def test_zero_images_and_no_predictions_give_nan(cuda):
    from jtsm_amd.evaluation import COCOEvaluator, COCOGroundTruth

    ev = COCOEvaluator(COCOGroundTruth(3), device=cuda)
    res = ev.evaluate()
    assert list(res) == ["bbox"] and list(res["bbox"]) == CR.METRICS and all(np.isnan(v) for v in res["bbox"].values())
    dataset = _boxes_dataset(np.random.default_rng(1), [[0], [0]])
    got, _ = _check(cuda, dataset, 1, kernels=False)
    assert all(np.isnan(v) for v in got["bbox"].values())


def test_tasks_are_inferred_from_pred_masks(cuda):
    from jtsm_amd.evaluation import COCOEvaluator

    dataset = _mask_dataset(np.random.default_rng(2), 20, 24, n_images=1)
    gt = _ground_truth(dataset, 2, True)
    for masks, tasks in ((False, ["bbox"]), (True, ["bbox", "segm"])):
        ev = COCOEvaluator(gt, device=cuda)
        ev.process([{"image_id": dataset[0]["image_id"]}], [{"instances": _instances(dataset[0], cuda, masks)}])
        assert list(ev.evaluate()) == tasks


def test_error_paths(cuda):
    from jtsm_amd import _lib as L
    from jtsm_amd.evaluation import COCOEvaluator

    dataset = _mask_dataset(np.random.default_rng(4), 20, 24, n_images=1)
    inst = _instances(dataset[0], cuda, True)
    ev = COCOEvaluator(_ground_truth(dataset, 2, True), device=cuda)
    with pytest.raises(ValueError, match="not in the ground truth"):
        ev.process([{"image_id": 12345}], [{"instances": inst}])
    ev = COCOEvaluator(_ground_truth(dataset, 2, False), tasks=("bbox", "segm"), device=cuda)
    with pytest.raises(ValueError, match="ground-truth masks"):
        ev.process([{"image_id": dataset[0]["image_id"]}], [{"instances": inst}])
    bad = _instances(dataset[0], cuda, False)
    bad.pred_classes[0] = 2                                           # outside [0, K)
    ev = COCOEvaluator(_ground_truth(dataset, 2, False), device=cuda)
    ev.process([{"image_id": dataset[0]["image_id"]}], [{"instances": bad}])
    with pytest.raises(ValueError, match="outside"):
        ev.evaluate()
    # beyond the key widths: JTSM_EINVAL with a message, nothing launched
    lib = L.lib()
    buf = torch.zeros(64, dtype=torch.float64, device=cuda)
    rc = lib.jtsm_coco_accumulate(None, 0, 1 << 15, 1 << 12, buf.data_ptr(), buf.data_ptr(), 101, buf.data_ptr(), 3,
                                  buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 1 << 20, L.stream())
    assert rc != 0 and b"sort key" in lib.jtsm_last_error()
    assert lib.jtsm_coco_image_workspace_bytes(1, 1, 1, 0, 0, 129) == 0
    rc = lib.jtsm_coco_image(None, None, None, None, 0, 0, 0, None, None, None, buf.data_ptr(), None, 0, 1, 0, 129,
                             buf.data_ptr(), buf.data_ptr(), None, buf.data_ptr(), buf.data_ptr(), None, None,
                             buf.data_ptr(), ctypes.c_size_t(512), L.stream())
    assert rc != 0 and b"rank bits" in lib.jtsm_last_error()


# ----------------------------------------------------------------------------------------- a real inference pass
def test_end_to_end_on_a_tiny_inference_pass(cuda):
    """The evaluator fed by DatasetEvaluators from a GeneralizedRCNN-style inference of the JTSM model (the recipe of
    tests/test_hip_inference.py): Instances as postprocessing leaves them on the device.  The ground truth is cut from
    the detections themselves (every fifth detection's box and mask, one of them a crowd region), so that there are
    matches; the restatement evaluates what is read back."""
    from model_util import jtsm_cfg, to_batched_inputs
    from oracle import model as OM

    from jtsm_amd.evaluation import COCOEvaluator, DatasetEvaluators
    from jtsm_amd.modeling import build_model

    torch.manual_seed(0)
    params = OM.init_params(seed=3, random_bn=True, input_gain=1.0 / 64)
    batch = OM.synthetic_batch(1234, B=2, size=256, R=160, sp_block=8)
    cfg = jtsm_cfg("cuda")
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = 1e-5
    cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST = 0.3
    model = build_model(cfg)
    model.load_state_dict({k: v.detach() for k, v in params.items()}, strict=True)
    model.eval()
    inputs = to_batched_inputs(batch)
    for i, inp in enumerate(inputs):
        inp["image_id"] = 9 - i
    with torch.no_grad():
        outputs = model(inputs)
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    dataset = []
    for inp, out in zip(inputs, outputs):
        inst = out["instances"]
        assert inst.pred_masks.dtype == torch.bool and len(inst) > 0
        boxes = inst.pred_boxes.tensor.cpu().numpy()
        masks = inst.pred_masks.cpu().numpy()
        classes = inst.pred_classes.cpu().numpy()
        pick = np.arange(0, len(boxes), 5)
        gb = boxes[pick].astype(np.float64)
        gb[:, 2:] -= gb[:, :2]
        dataset.append(dict(image_id=inp["image_id"], det_boxes=boxes, det_scores=inst.scores.cpu().numpy(),
                            det_classes=classes, det_masks=masks, gt_cats=classes[pick], gt_boxes=gb,
                            gt_area=masks[pick].reshape(len(pick), -1).sum(1).astype(np.float64),
                            gt_crowd=(np.arange(len(pick)) == 1).astype(np.uint8), gt_masks=masks[pick]))
    ev = DatasetEvaluators([COCOEvaluator(_ground_truth(dataset, K, True), device=cuda)])
    ev.reset()
    ev.process(inputs, outputs)
    got = ev.evaluate()
    want, _ = CR.evaluate(dataset, K, ("bbox", "segm"))
    assert list(got) == ["bbox", "segm"]
    for task in got:
        for k, v in want[task].items():
            assert _bits([got[task][k]])[0] == _bits([v])[0], (task, k, got[task][k], v)
        assert got[task]["AP"] > 0
