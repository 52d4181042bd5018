"""CPU suite: tests/pq_ref.py (the NumPy restatement of the panoptic-quality matching and of the semantic confusion
matrix and metrics) pinned on hand-worked cases whose expected integers and fractions are literals here; the host-side
pieces of jtsm_amd.evaluation that need no GPU (averaging, metrics, ground-truth constructors, DatasetEvaluators) and
the host side of the two entry points."""
import json
import math

import numpy as np
import pytest

import pq_ref as PR

THING_CAT, STUFF_CAT, NUM_CAT = [0, 1], [0, 1], 2          # category_id k of a thing / stuff row -> category k


def _row(sid, cat, isthing=1):
    return [sid, isthing, cat, -1, 0]


def _map(n, *runs):
    """n pixels, VOID but for (value, first, last) inclusive runs."""
    m = np.zeros(n, np.int32)
    for v, a, b in runs:
        m[a:b + 1] = v
    return m


def hand_cases():
    """name -> dict(shape, pred, pred_table, gt, gt_table, tp, fp, fn, iou: [(category, numerator, denominator)])."""
    c = {}
    # (a) 4x4, pixels row-major: A (cat 0) = 0-7, B (cat 1) = 8-13, 14-15 VOID; P1 (cat 0) = 0-5, P2 (cat 1) = 6-15.
    #     A-P1: 6 / (6 + 8 - 6 - 0) = 6/8; B-P2: 6 / (10 + 6 - 6 - 2) = 6/8
    c["a_two_matches"] = dict(shape=(4, 4), pred=_map(16, (1, 0, 5), (2, 6, 15)), pred_table=[_row(1, 0), _row(2, 1)],
                              gt=_map(16, (1, 0, 7), (2, 8, 13)), gt_table=[[0, 0], [1, 0]],
                              tp=[1, 1], fp=[0, 0], fn=[0, 0], iou=[(0, 6, 8), (1, 6, 8)])
    # (b) gt of 2 px inside a pred of 4 px, same category: 2 / (4 + 2 - 2) = 0.5 exactly, not above
    c["b_iou_exactly_half"] = dict(shape=(1, 6), pred=_map(6, (7, 0, 3)), pred_table=[_row(7, 0)],
                                   gt=_map(6, (1, 0, 1), (2, 2, 5)), gt_table=[[0, 0], [1, 0]],
                                   tp=[0, 0], fp=[1, 0], fn=[1, 1], iou=[])
    # (c) identical segments, different categories
    c["c_category_differs"] = dict(shape=(1, 4), pred=_map(4, (1, 0, 3)), pred_table=[_row(1, 1)],
                                   gt=_map(4, (1, 0, 3)), gt_table=[[0, 0]],
                                   tp=[0, 0], fp=[0, 1], fn=[1, 0], iou=[])
    # (d) an unmatched pred with 2 of 4 px on VOID is a false positive; with 4 of 6 px it is skipped
    c["d_half_on_void"] = dict(shape=(1, 8), pred=_map(8, (1, 0, 3)), pred_table=[_row(1, 0)],
                               gt=_map(8, (1, 2, 3)), gt_table=[[1, 0]],
                               tp=[0, 0], fp=[1, 0], fn=[0, 1], iou=[])
    c["d_more_than_half_on_void"] = dict(shape=(1, 8), pred=_map(8, (1, 0, 5)), pred_table=[_row(1, 0)],
                                         gt=_map(8, (1, 4, 7)), gt_table=[[1, 0]],
                                         tp=[0, 0], fp=[0, 0], fn=[0, 1], iou=[])
    # (e) two crowd rows of category 0: P1 lies on the first (not shielded), P2 on the last (shielded)
    c["e_last_crowd_row_shields"] = dict(shape=(2, 4), pred=_map(8, (1, 0, 3), (2, 4, 7)),
                                         pred_table=[_row(1, 0), _row(2, 0)],
                                         gt=_map(8, (1, 0, 3), (2, 4, 7)), gt_table=[[0, 1], [0, 1]],
                                         tp=[0, 0], fp=[1, 0], fn=[0, 0], iou=[])
    # (f) a gt row without a pixel is a false negative; a stuff row (isthing 0) matches exactly
    c["f_gt_row_without_pixels"] = dict(shape=(1, 4), pred=_map(4, (5, 0, 3)), pred_table=[_row(5, 0, isthing=0)],
                                        gt=_map(4, (1, 0, 3)), gt_table=[[0, 0], [1, 0]],
                                        tp=[1, 0], fp=[0, 0], fn=[0, 1], iou=[(0, 4, 4)])
    return c


def run_ref(case):
    return PR.pq_image(case["pred"], case["pred_table"], len(case["pred_table"]), THING_CAT, STUFF_CAT, case["gt"],
                       case["gt_table"], NUM_CAT)


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_restatement_on_hand_worked_cases(name):
    case = hand_cases()[name]
    r = run_ref(case)
    assert r["tp"].tolist() == case["tp"] and r["fp"].tolist() == case["fp"] and r["fn"].tolist() == case["fn"]
    assert r["stats"].tolist() == [0, 0, 0]
    assert r["matches"] == [(cat, num / den) for cat, num, den in case["iou"]]


def test_case_a_gives_pq_75_sq_75_rq_100():
    tot = PR.pq_accumulate([(c["pred"], c["pred_table"], 2, c["gt"], c["gt_table"]) for c in [hand_cases()["a_two_matches"]]],
                           THING_CAT, STUFF_CAT, NUM_CAT)
    assert tot["iou_sum"].tolist() == [0.75, 0.75] and tot["stats"].tolist() == [0, 0, 0, 1]
    res = PR.pq_result_dict(tot["tp"], tot["fp"], tot["fn"], tot["iou_sum"], [True, False])["panoptic_seg"]
    assert res == {"PQ": 75.0, "SQ": 75.0, "RQ": 100.0, "PQ_th": 75.0, "SQ_th": 75.0, "RQ_th": 100.0,
                   "PQ_st": 75.0, "SQ_st": 75.0, "RQ_st": 100.0}


def test_stats_words_and_num_pred():
    # pixel id 9 is in no row (2 px), row id 4 has no pixel, the row of category_id 5 maps to no category
    r = PR.pq_image(_map(6, (1, 0, 1), (9, 2, 3), (3, 4, 5)), [_row(1, 0), _row(4, 1), _row(3, 5)], 3, THING_CAT,
                    STUFF_CAT, _map(6, (1, 0, 1)), [[0, 0]], NUM_CAT)
    assert r["stats"].tolist() == [2, 1, 1] and r["tp"].tolist() == [1, 0] and r["fp"].tolist() == [0, 1]
    # only the first row counts: the second row's pixels name no row
    r = PR.pq_image(_map(4, (1, 0, 1), (2, 2, 3)), [_row(1, 0), _row(2, 0)], 1, THING_CAT, STUFF_CAT,
                    _map(4, (1, 0, 1)), [[0, 0]], NUM_CAT)
    assert r["stats"].tolist() == [2, 0, 0] and r["tp"].tolist() == [1, 0] and r["fp"].tolist() == [0, 0]


def test_pq_average_groups_and_empty_group():
    #            tp fp fn iou      pq             sq      rq
    # cat 0 (th): 2  1  1  1.5  -> 1.5 / 3 = .5,  .75,    2/3
    # cat 1 (th): 0  0  2  0    -> 0,             0,      0
    # cat 2 (st): 0  0  0       -> not counted
    r = PR.pq_average([2, 0, 0], [1, 0, 0], [1, 2, 0], [1.5, 0.0, 0.0], [True, True, False])
    assert r["All"] == {"pq": 0.25, "sq": 0.375, "rq": (2 / 3) / 2, "n": 2} and r["Things"] == r["All"]
    assert r["Stuff"]["n"] == 0 and all(math.isnan(r["Stuff"][k]) for k in ("pq", "sq", "rq"))
    from jtsm_amd.evaluation.panoptic_evaluation import pq_average

    mine = pq_average([2, 0, 0], [1, 0, 0], [1, 2, 0], [1.5, 0.0, 0.0], [True, True, False])
    for grp in ("All", "Things"):
        assert dict(mine[grp]) == r[grp]
    assert mine["Stuff"]["n"] == 0 and math.isnan(mine["Stuff"]["pq"])


def test_sem_seg_confusion_and_metrics():
    pred = np.array([[0, 0, 1, 1], [1, 0, 2, 1]])
    gt = np.array([[0, 1, 1, 255], [1, 0, 0, 1]])
    conf = PR.confusion(pred, gt, 3, 255)
    assert conf.tolist() == [[2, 1, 0, 0], [0, 3, 0, 1], [1, 0, 0, 0], [0, 0, 0, 0]]
    # (g) three classes, `c` in neither map: NaN for it, means over the two others
    conf = np.array([[3, 1, 0, 1], [1, 5, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]])
    res = PR.sem_seg_metrics(conf, ["a", "b", "c"])["sem_seg"]
    assert res["IoU-a"] == pytest.approx(100 * 3 / 5, rel=1e-14) and res["IoU-b"] == pytest.approx(100 * 5 / 7, rel=1e-14)
    assert res["ACC-a"] == pytest.approx(75.0, rel=1e-14) and res["ACC-b"] == pytest.approx(100 * 5 / 6, rel=1e-14)
    assert math.isnan(res["IoU-c"]) and math.isnan(res["ACC-c"])
    assert res["mIoU"] == pytest.approx(100 * (3 / 5 + 5 / 7) / 2, rel=1e-14)
    assert res["mACC"] == pytest.approx(100 * (3 / 4 + 5 / 6) / 2, rel=1e-14)
    assert res["fwIoU"] == pytest.approx(100 * (3 / 5 * 0.4 + 5 / 7 * 0.6), rel=1e-14)
    assert res["pACC"] == pytest.approx(80.0, rel=1e-14)
    # `c` predicted on one pixel but absent from the ground truth: still NaN, but mIoU now divides by three classes
    conf[2, 0] = 1
    res2 = PR.sem_seg_metrics(conf, ["a", "b", "c"])["sem_seg"]
    assert math.isnan(res2["IoU-c"]) and math.isnan(res2["ACC-c"])
    assert res2["IoU-a"] == pytest.approx(50.0, rel=1e-14)             # 3 / (5 + 4 - 3)
    assert res2["mIoU"] == pytest.approx(100 * (1 / 2 + 5 / 7) / 3, rel=1e-14)
    assert res2["mACC"] == pytest.approx(100 * (3 / 5 + 5 / 6) / 2, rel=1e-14)
    assert res2["fwIoU"] == pytest.approx(100 * (1 / 2 * 5 / 11 + 5 / 7 * 6 / 11), rel=1e-14)
    assert res2["pACC"] == pytest.approx(100 * 8 / 11, rel=1e-14)
    assert list(res2) == ["mIoU", "fwIoU", "IoU-a", "IoU-b", "IoU-c", "mACC", "pACC", "ACC-a", "ACC-b", "ACC-c"]
    # the product's host arithmetic gives the same floats
    from jtsm_amd.evaluation.sem_seg_evaluation import sem_seg_metrics

    for m in (conf, np.array([[3, 1, 0, 1], [1, 5, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]])):
        a, b = sem_seg_metrics(m, ["a", "b", "c"]), PR.sem_seg_metrics(m, ["a", "b", "c"])["sem_seg"]
        assert list(a) == list(b)
        for k in a:
            assert a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])), k


def test_lds_bounds_are_the_library_constants():
    from jtsm_amd import _lib
    from jtsm_amd.evaluation.panoptic_evaluation import PQ_LDS_CELLS
    from jtsm_amd.evaluation.sem_seg_evaluation import CONFUSION_LDS_CELLS

    lib = _lib.lib()
    assert lib.jtsm_pq_lds_cells() == PQ_LDS_CELLS == 16384
    assert lib.jtsm_confusion_lds_cells() == CONFUSION_LDS_CELLS == 128 * 128


def test_entry_points_check_their_arguments_on_the_host():
    """Argument errors are reported before anything is launched (no GPU is touched)."""
    import ctypes as C

    from jtsm_amd import _lib

    lib = _lib.lib()
    assert lib.jtsm_pq_accumulate_workspace_bytes(0, 0, 1) > 0
    assert lib.jtsm_pq_accumulate_workspace_bytes(20, 20, 133) % 256 == 0
    assert lib.jtsm_pq_accumulate_workspace_bytes(1 << 13, 1 << 13, 1) >= (((1 << 13) + 1) ** 2) * 4
    assert lib.jtsm_pq_accumulate_workspace_bytes(1 << 15, 1 << 15, 1) == 0           # beyond 2^28 counters
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    assert lib.jtsm_pq_accumulate(None, None, None, 0, None, 0, None, 0, None, None, 0, 0, 0, p, p, p, p, p, 0, None,
                                  0, None) != 0 and b"C=0" in lib.jtsm_last_error()
    assert lib.jtsm_pq_accumulate(None, None, None, 0, None, 0, None, 0, None, None, 0, 0, 1, p, p, p, p, p, 0, None,
                                  0, None) != 0 and b"workspace" in lib.jtsm_last_error()
    assert lib.jtsm_pq_accumulate(None, None, None, 3, None, 0, None, 0, None, None, 0, 0, 1, p, p, p, p, p, 0, p,
                                  1 << 20, None) != 0 and b"pred_table" in lib.jtsm_last_error()
    assert lib.jtsm_confusion_accumulate(p, p, 2, 16, 3, 255, p, p, 0, None) != 0
    assert b"gt_elem_bytes" in lib.jtsm_last_error()
    assert lib.jtsm_confusion_accumulate(p, p, 1, 16, 0, 255, p, p, 0, None) != 0
    assert lib.jtsm_confusion_accumulate(p, p, 1, 0, 3, 255, p, p, 0, None) == 0       # no pixels: nothing to do


def test_ground_truth_from_coco_panoptic_files(tmp_path):
    from PIL import Image

    from jtsm_amd.evaluation import PanopticGroundTruth

    ids = np.array([[70000, 70000, 5, 5], [70000, 999, 5, 0]], np.int64)       # 999 is not listed: VOID
    rgb = np.stack([ids % 256, ids // 256 % 256, ids // 65536], axis=-1).astype(np.uint8)
    Image.fromarray(rgb).save(str(tmp_path / "im7.png"))
    ann = {"annotations": [{"image_id": 7, "file_name": "im7.png", "segments_info": [
        {"id": 5, "category_id": 92, "iscrowd": 0, "area": 12345},
        {"id": 70000, "category_id": 1, "iscrowd": 1, "area": 1}]}]}
    (tmp_path / "gt.json").write_text(json.dumps(ann))
    gt = PanopticGroundTruth.from_coco_panoptic(str(tmp_path / "gt.json"), str(tmp_path), [1, {"id": 92, "isthing": 0}])
    assert gt.image_ids == [7] and 7 in gt
    seg_map, table = gt[7]
    assert seg_map.dtype == np.int32 and seg_map.tolist() == [[2, 2, 1, 1], [2, 0, 1, 0]]
    assert table.dtype == np.int32 and table.tolist() == [[1, 0], [0, 1]]
    ann["annotations"][0]["segments_info"][0]["category_id"] = 3
    (tmp_path / "bad.json").write_text(json.dumps(ann))
    with pytest.raises(ValueError, match="category"):
        PanopticGroundTruth.from_coco_panoptic(str(tmp_path / "bad.json"), str(tmp_path), [1, 92])
    same = PanopticGroundTruth.from_arrays([7], [seg_map], [table])
    assert same[7][0].tolist() == seg_map.tolist()


def test_dataset_evaluators_fan_out_and_merge():
    from jtsm_amd.evaluation import DatasetEvaluator, DatasetEvaluators

    class One(DatasetEvaluator):
        def __init__(self, key):
            self.key, self.seen, self.resets = key, [], 0

        def reset(self):
            self.resets += 1

        def process(self, inputs, outputs):
            self.seen.append((inputs, outputs))

        def evaluate(self):
            return None if self.key is None else {self.key: {"n": len(self.seen)}}

    a, b, c = One("x"), One("y"), One(None)
    both = DatasetEvaluators([a, b, c])
    both.reset()
    both.process([1], [2])
    assert a.resets == b.resets == 1 and a.seen == b.seen == c.seen == [([1], [2])]
    assert both.evaluate() == {"x": {"n": 1}, "y": {"n": 1}} and list(both.evaluate()) == ["x", "y"]
    with pytest.raises(AssertionError, match="x"):
        DatasetEvaluators([a, One("x")]).evaluate()
