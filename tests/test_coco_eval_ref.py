"""CPU suite: tests/coco_eval_ref.py — the NumPy / Python restatement of COCO box / mask AP — against
what the reference's own compiled cocoeval.cpp answered (tests/golden/coco_eval_reference.npz, recorded by
tests/golden/make_coco_eval_golden.py): the per-(category, area range, image) matches and ignore flags and the
precision / scores / recall tables, bit for bit.  No tolerance: every operation is one IEEE operation in a fixed order."""
import numpy as np
import pytest

import coco_eval_ref as CR
from conftest import load_cases

K = 6
CASES = load_cases("coco_eval_reference.npz")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def restated():
    out = {}
    for name, f in CASES.items():
        dataset = CR.dataset_from_fields(f)
        tasks = ("bbox", "segm") if "mask_hw" in f else ("bbox",)
        out[name] = (dataset,) + CR.evaluate(dataset, K, tasks, class_names=["c%d" % c for c in range(K)])
    return out


def test_the_recorded_cases_hold_what_they_must():
    assert sorted(CASES) == ["a", "b", "c", "d"]
    over_100 = with3 = without3 = False
    for name, f in CASES.items():
        ids = f["image_ids"].tolist()
        assert len(ids) <= 14 and ids != sorted(ids)
        assert (f["gt_cats"] == 3).sum() == 0 and (f["det_classes"] == 4).sum() == 0 and (f["gt_cats"] == 4).sum() > 0
        n3 = int((f["det_classes"] == 3).sum())
        with3, without3 = with3 or n3 > 0, without3 or n3 == 0
        start = np.concatenate([[0], np.cumsum(f["det_count"])])
        over_100 |= any(int((f["det_classes"][start[i]:start[i + 1]] == 0).sum()) > 100 for i in range(len(ids)))
        assert (f["gt_crowd"] == 1).any()
    assert over_100 and with3 and without3
    area = np.concatenate([f["gt_area"] for f in CASES.values()])
    assert (area < 32 ** 2).any() and ((area > 32 ** 2) & (area < 96 ** 2)).any() and (area > 96 ** 2).any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_and_ignore_flags_are_the_compiled_reference_s(restated, name):
    f = CASES[name]
    dataset, _, tables = restated[name]
    for task, tab in tables.items():
        sizes, matches, ignores, gt_ignores = CR.flatten_evals(tab["evals"], len(dataset), K)
        assert np.array_equal(sizes, f[task + "_sizes"]), task
        assert np.array_equal(matches, f[task + "_matches"]), task
        assert np.array_equal(ignores, f[task + "_ignores"]), task
        assert np.array_equal(gt_ignores, f[task + "_gt_ignores"]), task
        assert sizes[:, 0].max() == (100 if name in ("c", "d") else sizes[:, 0].max())   # truncated before matching


@pytest.mark.parametrize("name", sorted(CASES))
def test_tables_are_the_compiled_reference_s_bit_for_bit(restated, name):
    f = CASES[name]
    _, _, tables = restated[name]
    for task, tab in tables.items():
        for key in ("precision", "scores", "recall"):
            assert tab[key].shape == f["%s_%s" % (task, key)].shape
            assert np.array_equal(_bits(tab[key]), _bits(f["%s_%s" % (task, key)])), (task, key)


def test_summary_and_result_dict(restated):
    _, results, tables = restated["a"]
    assert list(results) == ["bbox", "segm"]
    for task in results:
        stats = tables[task]["stats"]
        assert stats.shape == (12,) and (stats[:3] >= 0).all()
        assert results[task]["AP"] == float(stats[0] * 100) and results[task]["AP75"] == float(stats[2] * 100)
        assert np.isnan(results[task]["AP-c3"])             # a category without ground truth: every entry is -1
        assert results[task]["AP-c4"] == 0.0                # ground truth and no detection: precision 0 everywhere
    # AP50 / AP75 pick rows 0 and 5 of the threshold axis: the linspace values equal the literals
    assert CR.IOU_THRS[0] == .5 and CR.IOU_THRS[5] == .75


def test_no_predictions_give_nan():
    dataset = CR.dataset_from_fields(CASES["c"])
    for im in dataset:
        im["det_boxes"], im["det_scores"], im["det_classes"] = im["det_boxes"][:0], im["det_scores"][:0], im["det_classes"][:0]
    results, _ = CR.evaluate(dataset, K)
    assert all(np.isnan(v) for v in results["bbox"].values()) and list(results["bbox"]) == CR.METRICS


def test_last_maximum_wins_among_equal_ious_and_crowd_matches_twice():
    gts = [dict(area=500.0, crowd=False), dict(area=500.0, crowd=False), dict(area=500.0, crowd=True)]
    dets = [dict(area=400.0), dict(area=400.0), dict(area=400.0)]
    ious = [[0.8, 0.8, 0.9], [0.1, 0.1, 0.7], [0.1, 0.1, 0.6]]
    m, ig, gig = CR.evaluate_image_category(dets, gts, ious, CR.AREA_RNG[0], CR.IOU_THRS)
    assert gig == [False, False, True]
    assert m[0] == [2, 3, 3] and ig[0] == [False, True, True]       # the second of the equal pair; the crowd twice
    assert m[9] == [0, 0, 0] and ig[9] == [False, False, False]     # 0.95: nothing reaches it; areas are in range


# ------------------------------------------------------------------------- host-side parts of the product (no GPU)
def test_key_widths_and_limits_are_refused_on_the_host():
    """The argument checks of the two entry points run before anything is launched: JTSM_EINVAL with a message."""
    from jtsm_amd import _lib as L

    lib = L.lib()
    assert lib.jtsm_coco_image_workspace_bytes(100, 7, 80, 480, 640, 100) > 100 * (480 * 640 // 8)
    assert lib.jtsm_coco_image_workspace_bytes(1, 1, 1, 0, 0, 129) == 0
    assert lib.jtsm_coco_accumulate_workspace_bytes(0, 80) > 0
    rc = lib.jtsm_coco_accumulate(None, 0, 1 << 15, 1 << 12, 8, 8, 101, 8, 3, 8, 8, 8, 256, 1 << 20, None)
    assert rc != 0 and b"sort key" in lib.jtsm_last_error()
    rc = lib.jtsm_coco_image(None, None, None, None, 0, 0, 0, None, None, None, 8, None, 0, 1, 0, 129, 8, 8, None, 8, 8,
                             None, None, 256, 512, None)
    assert rc != 0 and b"rank bits" in lib.jtsm_last_error()
    rc = lib.jtsm_coco_image(None, None, None, None, 0, 0, 0, None, None, None, 8, None, 5000, 1, 0, 100, 8, 8, None, 8,
                             8, None, None, 256, 512, None)
    assert rc != 0 and b"matched bits" in lib.jtsm_last_error()


def test_pack_masks_bit_order():
    from jtsm_amd.evaluation.coco_evaluation import pack_masks

    m = np.zeros((2, 3, 50), bool)
    m[0, 0, 0] = m[1, 2, 49] = m[1, 1, 13] = True
    w = pack_masks(m)
    assert w.shape == (2, 3) and w.dtype == np.uint64                    # 150 pixels: 3 words, a tail of 22 bits
    assert w[0].tolist() == [1, 0, 0] and w[1].tolist() == [1 << 63, 0, 1 << 21]   # pixels 63 and 149
    assert pack_masks(np.zeros((0, 4, 4), bool)).shape == (0, 1)


def test_ground_truth_loaders(tmp_path):
    import json

    from jtsm_amd.evaluation import COCOGroundTruth

    H, W = 4, 6
    mask = np.zeros((H, W), bool)
    mask[1:3, 2:5] = True
    runs, flat = [], mask.T.reshape(-1)                                   # column-major runs, starting with zeros
    value, count = False, 0
    for v in flat:
        if v == value:
            count += 1
        else:
            runs.append(count)
            value, count = v, 1
    runs.append(count)
    data = {"images": [{"id": 7, "height": H, "width": W}, {"id": 3, "height": H, "width": W}],
            "categories": [{"id": 18}, {"id": 5}],
            "annotations": [
                {"id": 1, "image_id": 7, "category_id": 5, "bbox": [2, 1, 3, 2], "area": 6.0, "iscrowd": 0,
                 "segmentation": {"size": [H, W], "counts": runs}},
                {"id": 2, "image_id": 7, "category_id": 18, "bbox": [0, 0, 2, 2], "area": 4.0, "iscrowd": 1,
                 "segmentation": {"size": [H, W], "counts": [H * W - 4, 4]}},
                {"id": 3, "image_id": 7, "category_id": 99, "bbox": [0, 0, 1, 1], "area": 1.0, "iscrowd": 0},
                {"id": 4, "image_id": 3, "category_id": 5, "bbox": [1, 1, 2, 2], "area": 3.5, "iscrowd": 0,
                 "segmentation": [[1, 1, 3, 1, 3, 3]]}]}
    path = tmp_path / "instances.json"
    path.write_text(json.dumps(data))
    gt = COCOGroundTruth.from_coco_json(str(path), [18, 5])
    assert gt.image_ids == [3, 7] and gt.num_categories == 2
    it = gt[7]                                                          # sorted by category index: 18 -> 0, 5 -> 1
    assert it["cats"].tolist() == [0, 1] and it["iscrowd"].tolist() == [1, 0] and it["area"].tolist() == [4.0, 6.0]
    assert it["cat_start"].tolist() == [0, 1, 2] and it["boxes"][1].tolist() == [2.0, 1.0, 3.0, 2.0]
    assert it["mask_shape"] == (H, W) and gt.has_masks(7)
    bits = np.unpackbits(it["words"].view(np.uint8), axis=1, bitorder="little")[:, :H * W].reshape(2, H, W)
    assert np.array_equal(bits[1].astype(bool), mask) and bits[0].sum() == 4 and bits[0][2:, 5].all()
    assert not gt.has_masks(3) and "annotation id 4" in gt.missing_masks[3]       # a polygon and no loader
    gt2 = COCOGroundTruth.from_coco_json(str(path), [{"id": 18}, {"id": 5}], mask_loader=lambda ann: mask)
    assert gt2.has_masks(3) and gt2[3]["area"].tolist() == [3.5]
    dicts = [{"image_id": 1, "annotations": [
        {"category_id": 1, "bbox": [2, 1, 5, 3], "segmentation": mask, "iscrowd": 0},
        {"category_id": 0, "bbox": [0, 0, 2, 2], "bbox_mode": 1, "segmentation": mask, "area": 9.0}]},
        {"image_id": 0, "annotations": []}]
    gt3 = COCOGroundTruth.from_dataset_dicts(dicts, 2)
    assert gt3.image_ids == [0, 1] and gt3[1]["cats"].tolist() == [0, 1] and gt3[1]["area"].tolist() == [9.0, 6.0]
    assert gt3[1]["boxes"].tolist() == [[0.0, 0.0, 2.0, 2.0], [2.0, 1.0, 3.0, 2.0]] and gt3.has_masks(1) and gt3.has_masks(0)
