"""CPU suite: tests/coco_keypoint_ref.py — the NumPy restatement of the COCO keypoints task — against
what the reference's own compiled cocoeval.cpp answered when it was fed the restatement's OKS rows and the separate
is_crowd / ignore flags (tests/golden/coco_keypoint_reference.npz, recorded by
tests/golden/make_coco_keypoint_golden.py): matches, ignore flags and tables bit for bit.  The OKS itself is checked
against hand-worked values, and the recorded cases' margin condition — every OKS at least 1e-9 from each threshold and
from every other OKS of its detection and category — is asserted again from the fixture: with it a rounding
difference in OKS (another exp, another summation order) cannot move a match."""
import json

import numpy as np
import pytest

import coco_eval_ref as CR
import coco_keypoint_ref as KR
from conftest import load_cases

K = 4
CASES = load_cases("coco_keypoint_reference.npz")
NAMES = ["c%d" % c for c in range(K)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def restated():
    out = {}
    for name, f in CASES.items():
        dataset, sigmas, processed = KR.dataset_from_fields(f)
        out[name] = (dataset, sigmas, processed) + KR.evaluate(dataset, K, sigmas, class_names=NAMES)
    return out


def test_the_recorded_cases_hold_what_they_must(restated):
    assert sorted(CASES) == ["p17", "p5"]
    assert len(CASES["p5"]["sigmas"]) == 5 and len(CASES["p17"]["sigmas"]) == 17
    assert np.array_equal(CASES["p17"]["sigmas"], KR.COCO_SIGMAS) and CASES["p5"]["sigmas"].max() != KR.COCO_SIGMAS.max()
    for name, f in CASES.items():
        dataset, sigmas, processed, _, tab = restated[name]
        ids = f["image_ids"].tolist()
        assert 3 <= len(ids) <= 5 and ids != sorted(ids)
        assert f["det_count"].max() <= 30 and f["gt_count"].max() <= 70
        assert any(int((im["det_classes"] == 0).sum()) > 20 for im in dataset)
        assert any(int((im["gt_cats"] == 0).sum()) > 64 for im in dataset)
        assert (f["gt_cats"] == 3).sum() == 0 and (f["det_classes"] == 3).sum() > 0
        assert (f["det_classes"] == 2).sum() == 0 and (f["gt_cats"] == 2).sum() > 0
        area = f["gt_area"]
        assert (area < 32 ** 2).any() and ((area > 32 ** 2) & (area < 96 ** 2)).any() and (area > 96 ** 2).any()
        assert not processed.all() and all(len(im["det_scores"]) == 0 for im, p in zip(dataset, processed) if not p)
        crowd, nk = f["gt_crowd"] != 0, f["gt_num_keypoints"]
        assert (crowd & (nk > 0)).any() and (~crowd & (nk == 0)).any()
        assert ((f["gt_keypoints"][:, :, 2] > 0).sum(1) == nk).all()
        flat = [v for info in tab["per_image"] for rows in info["ious"].values() for row in rows for v in row]
        assert flat.count(1.0) >= 3 and 0 < min(flat) < 0.5          # exact matches; nothing sinks to zero
        # the margin condition
        to_thr, to_other = KR.margins(tab["per_image"], dataset, tab["order"])
        print(name, "least distance of an OKS from a threshold %.3g, from another OKS %.3g" % (to_thr, to_other))
        assert to_thr >= KR.MARGIN and to_other >= KR.MARGIN


@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_and_ignore_flags_are_the_compiled_reference_s(restated, name):
    f = CASES[name]
    dataset, _, _, _, tab = restated[name]
    sizes, matches, ignores, gt_ignores = CR.flatten_evals(tab["evals"], len(dataset), K, num_areas=len(KR.AREA_RNG))
    assert np.array_equal(sizes, f["kp_sizes"]) and sizes[:, 0].max() == 20             # truncated before matching
    assert np.array_equal(matches, f["kp_matches"])
    assert np.array_equal(ignores, f["kp_ignores"])
    assert np.array_equal(gt_ignores, f["kp_gt_ignores"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_tables_are_the_compiled_reference_s_bit_for_bit(restated, name):
    f = CASES[name]
    _, _, _, result, tab = restated[name]
    for key in ("precision", "scores", "recall"):
        assert tab[key].shape == f["kp_" + key].shape
        assert np.array_equal(_bits(tab[key]), _bits(f["kp_" + key])), key
    assert tab["precision"].shape == (10, 101, K, 3, 1) and tab["recall"].shape == (10, K, 3, 1)
    assert tab["stats"].shape == (10,) and list(result)[:5] == KR.METRICS
    assert result["AP"] == float(tab["stats"][0] * 100) > 0 and result["APl"] == float(tab["stats"][4] * 100)
    assert np.isnan(result["AP-c3"]) and result["AP-c2"] == 0.0     # no ground truth: -1 everywhere; no detection: 0


def test_a_matcher_with_one_flag_decides_the_recorded_cases_otherwise(restated):
    """ignore := iscrowd or num_keypoints == 0, but only a crowd may be matched twice: with `crowd := ignore` the
    unlabelled object takes a second detection and the recorded matches are missed."""
    for name, f in CASES.items():
        dataset, sigmas, _, _, tab = restated[name]
        merged = [dict(im, gt_crowd=((im["gt_crowd"] != 0) | (im["gt_num_keypoints"] == 0)).astype(np.uint8))
                  for im in dataset]
        _, evals, _ = KR.evaluate_images(merged, K, sigmas)
        _, matches, ignores, gt_ignores = CR.flatten_evals(evals, len(dataset), K, num_areas=len(KR.AREA_RNG))
        assert np.array_equal(gt_ignores, f["kp_gt_ignores"])
        assert not np.array_equal(matches, f["kp_matches"]) and not np.array_equal(ignores, f["kp_ignores"])


# ------------------------------------------------------------------------------------------- hand-worked OKS
def _oks(det_xy, gt_kp, sigmas, area, box=(0.0, 0.0, 10.0, 10.0)):
    """OKS of one detection whose points the evaluation sees at det_xy (the model's output lies 0.5 above them)."""
    P = len(sigmas)
    det = np.concatenate([np.asarray(det_xy, np.float64) + 0.5, np.ones((P, 1))], 1).astype(np.float32)
    image = dict(det_boxes=np.array([[0, 0, 10, 10]], np.float32), det_scores=np.array([0.5], np.float32),
                 det_classes=np.array([0]), det_keypoints=det[None])
    gt = dict(keypoints=np.asarray(gt_kp, np.float64).flatten().tolist(), bbox=list(box), area=area)
    return float(KR.compute_oks(KR.detections_of(image), [gt], sigmas)[0, 0])


def test_hand_worked_oks_values():
    sig = np.array([0.05, 0.08, 0.1])
    gt = np.array([[10.0, 20.0, 2.0], [30.25, 40.5, 1.0], [50.0, 60.0, 0.0]])
    eps = 2.220446049250313e-16
    assert np.spacing(1) == eps
    # identical points (the unlabelled third is anywhere)
    assert _oks([[10.0, 20.0], [30.25, 40.5], [0.0, 0.0]], gt, sig, 900.0) == 1.0
    # one visible keypoint, displaced by d = 5 (3 along x, 4 along y)
    one = np.array([[10.0, 20.0, 0.0], [30.0, 40.0, 2.0], [50.0, 60.0, 0.0]])
    got = _oks([[0.0, 0.0], [33.0, 44.0], [9.0, 9.0]], one, sig, 900.0)
    want = np.exp(-(5.0 ** 2) / (2 * (2 * 0.08) ** 2 * (900.0 + eps)))
    assert abs(got - want) <= 1e-15, (got, want)
    # two visible keypoints: the mean over the visible ones only
    got = _oks([[10.0, 23.0], [30.25, 40.5], [0.0, 0.0]], gt, sig, 400.0)
    want = (np.exp(-9.0 / (2 * (2 * 0.05) ** 2 * (400.0 + eps))) + 1.0) / 2
    assert abs(got - want) <= 1e-15, (got, want)
    # no labelled keypoint: the distance to the doubled box [-10, 20] x [-10, 20], the mean over all three
    none = np.array([[1.0, 1.0, 0.0], [2.0, 2.0, 0.0], [3.0, 3.0, 0.0]])
    assert _oks([[-10.0, 20.0], [5.0, 5.0], [19.5, -9.5]], none, sig, 100.0) == 1.0
    got = _oks([[-12.0, 5.0], [5.0, 5.0], [5.0, 23.0]], none, sig, 100.0)
    want = (np.exp(-4.0 / (2 * (2 * 0.05) ** 2 * (100.0 + eps))) + 1.0
            + np.exp(-9.0 / (2 * (2 * 0.1) ** 2 * (100.0 + eps)))) / 3
    assert abs(got - want) <= 1e-15, (got, want)


def test_the_shift_is_taken_in_fp32_on_a_copy():
    kp = np.array([[[0.1, 16777216.0, 0.7]]], np.float32)          # 2^24 - 0.5 is no fp32 number: it rounds to 2^24
    image = dict(det_boxes=np.zeros((1, 4), np.float32), det_scores=np.ones(1, np.float32), det_classes=np.zeros(1, int),
                 det_keypoints=kp)
    before = kp.copy()
    got = KR.detections_of(image)[0]["keypoints"]
    assert got == [float(np.float32(0.1) - np.float32(0.5)), 16777216.0, float(np.float32(0.7))]
    assert np.array_equal(kp, before)


def test_summary_picks_the_keypoint_rows():
    rng = np.random.default_rng(0)
    p, r = rng.random((10, 101, 2, 3, 1)), rng.random((10, 2, 3, 1))
    p[:, :, 1, 2] = -1
    s = KR.summarize(p, r)
    assert s[0] == np.mean(p[:, :, :, 0, 0]) and s[1] == np.mean(p[0, :, :, 0, 0]) and s[2] == np.mean(p[5, :, :, 0, 0])
    assert s[3] == np.mean(p[:, :, :, 1, 0]) and s[4] == np.mean(p[:, :, 0, 2, 0])
    assert s[5] == np.mean(r[:, :, 0, 0]) and s[6] == np.mean(r[0, :, 0, 0]) and s[9] == np.mean(r[:, :, 2, 0])


# ------------------------------------------------------------------------- host-side parts of the product (no GPU)
def test_product_constants_and_summary_are_the_restatement_s():
    from jtsm_amd.evaluation import coco_evaluation as CE

    assert CE.KP_MAX_DETS == KR.MAX_DETS and CE.KP_AREA_RNG == KR.AREA_RNG and CE.KP_METRICS == KR.METRICS
    assert np.array_equal(_bits(CE.COCO_KPT_OKS_SIGMAS), _bits(KR.COCO_SIGMAS))
    rng = np.random.default_rng(1)
    p, r = rng.random((10, 101, 3, 3, 1)), rng.random((10, 3, 3, 1))
    p[:, :, 2] = -1
    r[:, 2] = -1
    assert np.array_equal(_bits(CE.summarize_keypoints(p, r)), _bits(KR.summarize(p, r)))
    names = ["a", "b", "c"]
    got, want = CE.derive_coco_results(KR.summarize(p, r), p, names, CE.KP_METRICS), KR.derive_results(KR.summarize(p, r), p, names)
    assert list(got) == list(want) and all(_bits([got[k]])[0] == _bits([want[k]])[0] for k in want)
    assert list(CE.derive_coco_results(None, None, metrics=CE.KP_METRICS)) == KR.METRICS


def test_limits_are_refused_on_the_host():
    from jtsm_amd import _lib as L

    lib = L.lib()
    assert lib.jtsm_coco_image_keypoints_workspace_bytes(20, 7, 1, 17, 20) == lib.jtsm_coco_image_workspace_bytes(20, 7, 1, 0, 0, 20) > 0
    assert lib.jtsm_coco_image_keypoints_workspace_bytes(20, 7, 1, 65, 20) == 0
    assert lib.jtsm_coco_image_keypoints_workspace_bytes(20, 7, 1, 0, 20) == 0
    call = lambda P, G=0, max_det=20: lib.jtsm_coco_image_keypoints(  # noqa: E731
        None, None, None, None, 0, P, None, None, None, None, None, 8, G, 1, 8, 0, max_det, 8, 8, None, 8, 8, None, None,
        256, 512, None)
    assert call(65) != 0 and b"keypoints" in lib.jtsm_last_error()
    assert call(17, max_det=129) != 0 and b"rank bits" in lib.jtsm_last_error()
    assert call(17, G=5000) != 0


def test_ground_truth_ingestion(tmp_path):
    from jtsm_amd.evaluation import COCOGroundTruth

    kp_a = [10, 20, 2, 30, 40, 1, 0, 0, 0]
    kp_b = [[5.5, 6.5, 0], [7.0, 8.0, 0], [1.0, 2.0, 0]]
    # dataset dicts: x and y minus 0.5, num_keypoints from the field or counted; the annotation is left alone
    dicts = [{"image_id": 4, "annotations": [
        {"category_id": 1, "bbox": [0, 0, 50, 50], "keypoints": list(kp_a)},
        {"category_id": 0, "bbox": [0, 0, 9, 9], "keypoints": kp_b, "num_keypoints": 3}]},
        {"image_id": 2, "annotations": [{"category_id": 0, "bbox": [0, 0, 9, 9], "keypoints": list(kp_a)},
                                        {"category_id": 0, "bbox": [1, 1, 9, 9]}]},
        {"image_id": 9, "annotations": []}]
    gt = COCOGroundTruth.from_dataset_dicts(dicts, 2)
    it = gt[4]                                                           # sorted by category: the second comes first
    assert it["cats"].tolist() == [0, 1] and it["num_keypoints"].tolist() == [3, 2]
    assert it["keypoints"].dtype == np.float64 and it["keypoints"].shape == (2, 3, 3)
    assert it["keypoints"][0].tolist() == [[5.0, 6.0, 0.0], [6.5, 7.5, 0.0], [0.5, 1.5, 0.0]]
    assert it["keypoints"][1].tolist() == [[9.5, 19.5, 2.0], [29.5, 39.5, 1.0], [-0.5, -0.5, 0.0]]
    assert dicts[0]["annotations"][0]["keypoints"] == kp_a
    assert gt.has_keypoints(4) and gt.has_keypoints(9) and not gt.has_keypoints(2)
    assert gt[2]["keypoints"] is None and "annotation 1 of image 2" in gt.missing_keypoints[2]
    # a COCO file: as they stand
    data = {"images": [{"id": 1, "height": 60, "width": 60}, {"id": 8, "height": 60, "width": 60}],
            "annotations": [
                {"id": 11, "image_id": 1, "category_id": 7, "bbox": [0, 0, 50, 50], "area": 2000.0, "iscrowd": 0,
                 "keypoints": kp_a, "num_keypoints": 2},
                {"id": 12, "image_id": 1, "category_id": 7, "bbox": [0, 0, 50, 50], "area": 2100.0, "iscrowd": 1,
                 "keypoints": [0] * 9},
                {"id": 13, "image_id": 8, "category_id": 7, "bbox": [0, 0, 5, 5], "area": 20.0, "iscrowd": 0}]}
    path = tmp_path / "person_keypoints.json"
    path.write_text(json.dumps(data))
    gt = COCOGroundTruth.from_coco_json(str(path), [7])
    assert gt[1]["keypoints"][0].tolist() == [[10.0, 20.0, 2.0], [30.0, 40.0, 1.0], [0.0, 0.0, 0.0]]
    assert gt[1]["num_keypoints"].tolist() == [2, 0] and gt.has_keypoints(1)
    assert not gt.has_keypoints(8) and "annotation id 13" in gt.missing_keypoints[8]
    # arrays: the default num_keypoints is the count of v > 0, and both follow the category sort
    gt = COCOGroundTruth.from_arrays([3], [[1, 0]], [np.zeros((2, 4))], [[5.0, 6.0]], [[0, 0]], 2,
                                     keypoints=[np.array([np.reshape(kp_a, (3, 3)), np.array(kp_b)])])
    assert gt[3]["num_keypoints"].tolist() == [0, 2] and gt[3]["keypoints"][1].tolist() == np.reshape(kp_a, (3, 3)).tolist()
    with pytest.raises(ValueError, match="keypoints"):
        COCOGroundTruth.from_dataset_dicts([{"image_id": 1, "annotations": [
            {"category_id": 0, "bbox": [0, 0, 1, 1], "keypoints": [1, 1, 1]},
            {"category_id": 0, "bbox": [0, 0, 1, 1], "keypoints": [1, 1, 1, 2, 2, 2]}]}], 1)
