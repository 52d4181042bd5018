"""GPU suite (pytest -m gpu): the keypoints task of the device-side COCO evaluator (jtsm_coco_image_keypoints in
jtsm_amd/csrc/coco_eval.hip, jtsm_amd/evaluation/coco_evaluation.py) against tests/coco_keypoint_ref.py, the NumPy
restatement of DESIGN.md §4g, and against what the reference's compiled cocoeval.cpp recorded
(tests/golden/coco_keypoint_reference.npz).

OKS: the `ious` debug matrix within 1e-12 absolute of the restatement — a mean of at most 64 terms in [0, 1], each an
fp64 exp of an argument with a handful of roundings, summed in keypoint order where NumPy sums pairwise: an error near
1e-14.  Everything after it exactly: the ranks, the matched / ignore words of every record, npos, the precision /
scores / recall tables as fp64 bit patterns and the result dictionary; the recorded cases keep every OKS 1e-9 away from
the thresholds and from the other OKS of its detection (tests/test_coco_keypoint_ref.py), so the OKS error cannot move
a match."""
import numpy as np
import pytest
import torch

import coco_eval_ref as CR
import coco_keypoint_ref as KR
from conftest import load_cases

pytestmark = pytest.mark.gpu

K = 4
NAMES = ["c%d" % c for c in range(K)]
OKS_TOLERANCE = 1e-12
RECORD = np.dtype([("cat", "<i4"), ("image", "<i4"), ("rank", "<i4"), ("score", "<f4"), ("matched", "<u8"),
                   ("ignore", "<u8")])
CASES = load_cases("coco_keypoint_reference.npz")
_RESTATED = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want):
    return list(got) == list(want) and all(_bits([got[k]])[0] == _bits([want[k]])[0] for k in want)


def _restated(name):
    """(dataset, sigmas, processed, result, tables) of a recorded case: computed once, shared, left unchanged."""
    if name not in _RESTATED:
        dataset, sigmas, processed = KR.dataset_from_fields(CASES[name])
        _RESTATED[name] = (dataset, sigmas, processed) + KR.evaluate(dataset, K, sigmas, class_names=NAMES)
    return _RESTATED[name]


def _ground_truth(dataset, num_categories):
    from jtsm_amd.evaluation import COCOGroundTruth

    col = lambda key: [im[key] for im in dataset]  # noqa: E731
    return COCOGroundTruth.from_arrays(col("image_id"), col("gt_cats"), col("gt_boxes"), col("gt_area"), col("gt_crowd"),
                                       num_categories, keypoints=col("gt_keypoints"),
                                       num_keypoints=col("gt_num_keypoints"))


def _instances(image, cuda, keypoints=True):
    from jtsm_amd.structures import Boxes, Instances

    up = lambda key, dt: torch.from_numpy(np.ascontiguousarray(image[key], dt)).to(cuda)  # noqa: E731
    inst = Instances((256, 256), pred_boxes=Boxes(up("det_boxes", np.float32).reshape(-1, 4)),
                     scores=up("det_scores", np.float32), pred_classes=up("det_classes", np.int64))
    if keypoints:
        inst.set("pred_keypoints", up("det_keypoints", np.float32))
    return inst


def _evaluator(cuda, name, **kw):
    from jtsm_amd.evaluation import COCOEvaluator

    dataset, sigmas, _, _, _ = _restated(name)
    custom = () if np.array_equal(sigmas, KR.COCO_SIGMAS) else tuple(sigmas.tolist())     # empty: the COCO default
    return COCOEvaluator(_ground_truth(dataset, K), class_names=NAMES, device=cuda, kpt_oks_sigmas=custom, **kw)


# ------------------------------------------------------------------------------------------------ recorded cases
@pytest.mark.parametrize("name", sorted(CASES))
def test_evaluator_matches_the_restatement_and_the_compiled_reference(cuda, name):
    f = CASES[name]
    dataset, sigmas, processed, want, tab = _restated(name)
    ev = _evaluator(cuda, name, tasks=("keypoints",))
    ev.reset()
    for im, shown in zip(dataset, processed):
        if not shown:                                       # its ground truth still counts
            continue
        inst = _instances(im, cuda)
        before = inst.pred_keypoints.clone()
        ev.process([{"image_id": im["image_id"]}], [{"instances": inst}])
        assert torch.equal(inst.pred_keypoints.view(torch.int32), before.view(torch.int32))
    got = ev.evaluate()
    assert list(got) == ["keypoints"] and _same(got["keypoints"], want), (got, want)
    assert list(got["keypoints"])[:5] == KR.METRICS and got["keypoints"]["AP"] > 0 and np.isnan(got["keypoints"]["AP-c3"])
    last = ev.last_eval["keypoints"]
    assert last["precision"].shape == last["scores"].shape == (10, 101, K, 3, 1) and last["recall"].shape == (10, K, 3, 1)
    assert np.array_equal(last["npos"], tab["npos"]) and last["stats"].shape == (10,)
    for key in ("precision", "scores", "recall"):
        assert np.array_equal(_bits(last[key]), _bits(tab[key])), key
        assert np.array_equal(_bits(last[key]), _bits(f["kp_" + key])), key          # the compiled reference's
    assert np.array_equal(_bits(last["stats"]), _bits(tab["stats"]))
    assert _same(ev.evaluate()["keypoints"], want)                                  # a second time: the same


@pytest.mark.parametrize("name", sorted(CASES))
def test_oks_ranks_and_record_words_of_every_image(cuda, name):
    from jtsm_amd.evaluation import coco_evaluation as CE

    dataset, sigmas, _, _, tab = _restated(name)
    # the restatement's matches and flags, which the record words are held to below, are the compiled reference's
    _, matches, ignores, gt_ignores = CR.flatten_evals(tab["evals"], len(dataset), K, num_areas=len(KR.AREA_RNG))
    f = CASES[name]
    assert np.array_equal(matches, f["kp_matches"]) and np.array_equal(ignores, f["kp_ignores"])
    assert np.array_equal(gt_ignores, f["kp_gt_ignores"])
    gt = _ground_truth(dataset, K)
    index ={image_id: i for i, image_id in enumerate(gt.image_ids)}
    state = CE.new_state(K, cuda, keypoints=True)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    dev_sigmas = up(np.asarray(sigmas, np.float64))
    worst = 0.0
    for j, im in enumerate(dataset):
        i = index[im["image_id"]]
        assert tab["order"][i] == j
        item = gt[im["image_id"]]
        ignore = ((item["iscrowd"] != 0) | (item["num_keypoints"] == 0)).astype(np.uint8)
        g = dict(boxes=up(item["boxes"]), area=up(item["area"]), iscrowd=up(item["iscrowd"]), ignore=up(ignore),
                 keypoints=up(item["keypoints"]), cat_start=up(item["cat_start"]))
        inst = _instances(im, cuda)
        out = CE.coco_image_keypoints(inst.pred_boxes.tensor, inst.scores, inst.pred_classes.to(torch.int32),
                                      inst.pred_keypoints, g, dev_sigmas, i, state, with_debug=True)
        info = tab["per_image"][i]
        assert np.array_equal(out["rank"].cpu().numpy(), info["rank"]), j
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
                err = float(np.abs(ious[np.ix_(rows, cols)] - w).max())
                worst = max(worst, err)
                assert err <= OKS_TOLERANCE, (j, c, err)
                assert np.array_equal(ious[np.ix_(rows, cols)] == 1.0, w == 1.0)     # e = 0 is exact on both sides
                same[np.ix_(rows, cols)] = True
            m, ig = KR.match_bits(tab["evals"], i, c, len(rows))
            assert rec["matched"][rows].tolist() == m and rec["ignore"][rows].tolist() == ig, (j, c)
        assert (ious[~same] == -1.0).all()
        assert (rec["matched"][~kept] == 0).all() and (rec["ignore"][~kept] == 0).all()
    print(name, "largest |OKS - restatement| = %.3g" % worst)
    npos = state["npos"].cpu().numpy()
    assert np.array_equal(npos[:, :3], tab["npos"]) and np.array_equal(npos[:, 3], npos[:, 2])


# ------------------------------------------------------------------------------------------------- the interface
def test_tasks_are_inferred_from_pred_keypoints(cuda):
    dataset, _, _, want, _ = _restated("p5")
    for keypoints, tasks in ((False, ["bbox"]), (True, ["bbox", "keypoints"])):
        ev = _evaluator(cuda, "p5")
        ev.process([{"image_id": dataset[0]["image_id"]}], [{"instances": _instances(dataset[0], cuda, keypoints)}])
        assert list(ev.evaluate()) == tasks
    ev = _evaluator(cuda, "p5")                              # the whole case with both tasks: keypoints as alone
    for im in dataset[:3]:
        ev.process([{"image_id": im["image_id"]}], [{"instances": _instances(im, cuda)}])
    got = ev.evaluate()
    assert list(got) == ["bbox", "keypoints"] and _same(got["keypoints"], want)
    assert len(got["bbox"]) == 6 + K and ev.last_eval["bbox"]["precision"].shape == (10, 101, K, 4, 3)


def test_error_paths(cuda):
    from jtsm_amd.evaluation import COCOEvaluator, COCOGroundTruth

    dataset, sigmas, _, _, _ = _restated("p5")
    im = dataset[0]
    one = [{"image_id": im["image_id"]}], [{"instances": _instances(im, cuda)}]
    ev = COCOEvaluator(_ground_truth(dataset, K), tasks=("keypoints",), device=cuda)      # 17 sigmas, 5 keypoints
    with pytest.raises(ValueError, match="numbers of keypoints differ"):
        ev.process(*one)
    ev = COCOEvaluator(_ground_truth(dataset, K), tasks=("keypoints",), device=cuda, kpt_oks_sigmas=[0.1] * 4)
    with pytest.raises(ValueError, match="numbers of keypoints differ"):
        ev.process(*one)
    col = lambda key: [x[key] for x in dataset]  # noqa: E731
    bare = COCOGroundTruth.from_arrays(col("image_id"), col("gt_cats"), col("gt_boxes"), col("gt_area"),
                                       col("gt_crowd"), K)
    ev = COCOEvaluator(bare, tasks=("keypoints",), device=cuda, kpt_oks_sigmas=sigmas)
    with pytest.raises(ValueError, match="ground-truth keypoints"):
        ev.process(*one)
    ev = COCOEvaluator(_ground_truth(dataset, K), tasks=("keypoints",), device=cuda, kpt_oks_sigmas=sigmas)
    with pytest.raises(ValueError, match="needs pred_keypoints"):
        ev.process(one[0], [{"instances": _instances(im, cuda, False)}])
    res = ev.evaluate()                                                              # no prediction at all
    assert list(res["keypoints"]) == KR.METRICS and all(np.isnan(v) for v in res["keypoints"].values())


# ----------------------------------------------------------------------------------------- a real inference pass
def test_end_to_end_on_a_tiny_keypoint_rcnn(cuda):
    """The evaluator fed by DatasetEvaluators from the inference of the 5-keypoint Keypoint R-CNN of
    tests/test_hip_keypoint_model.py on its two 128 x 128 images: Instances as the model leaves them on the device.
    The ground truth of an image is its top detection (box, class and the points the evaluation sees, the first
    unlabelled), so that there are matches; the restatement evaluates what is read back."""
    import test_hip_keypoint_model as TK

    from jtsm_amd.evaluation import COCOEvaluator, DatasetEvaluators

    model = TK.build(TK.keypoint_cfg())
    model.eval()
    data = TK.batch(None)
    results = model.inference(data, do_postprocess=False)
    sigmas = [0.03, 0.05, 0.07, 0.09, 0.11]
    inputs, outputs, dataset = [], [], []
    for i, r in enumerate(results):
        assert tuple(r.pred_keypoints.shape[1:]) == (TK.K, 3) and r.pred_keypoints.dtype == torch.float32
        boxes, kp = r.pred_boxes.tensor.cpu().numpy(), r.pred_keypoints.cpu().numpy()
        scores, classes = r.scores.cpu().numpy(), r.pred_classes.cpu().numpy()
        top = np.argsort(-scores, kind="stable")[:1]
        gb = boxes[top].astype(np.float64)
        gb[:, 2:] -= gb[:, :2]
        gk = kp[top].copy()
        gk[:, :, :2] -= np.float32(0.5)
        gk[:, :, 2] = 2.0
        gk[:, 0, 2] = 0.0
        inputs.append({"image_id": 40 - i})
        outputs.append({"instances": r})
        dataset.append(dict(image_id=40 - i, det_boxes=boxes, det_scores=scores, det_classes=classes, det_masks=None,
                            det_keypoints=kp, gt_cats=classes[top], gt_boxes=gb, gt_area=gb[:, 2] * gb[:, 3],
                            gt_crowd=np.zeros(len(top), np.uint8), gt_masks=None, gt_keypoints=gk.astype(np.float64),
                            gt_num_keypoints=np.full(len(top), TK.K - 1)))
    assert sum(len(im["det_scores"]) for im in dataset) > 0
    before = [r.pred_keypoints.clone() for r in results]
    ev = DatasetEvaluators([COCOEvaluator(_ground_truth(dataset, 3), device=cuda, kpt_oks_sigmas=sigmas)])
    ev.reset()
    ev.process(inputs, outputs)
    got = ev.evaluate()
    want, tab = KR.evaluate(dataset, 3, np.array(sigmas))
    assert list(got) == ["bbox", "keypoints"] and _same(got["keypoints"], want), (got, want)
    assert got["keypoints"]["AP"] > 0
    flat = [v for info in tab["per_image"] for rows in info["ious"].values() for row in rows for v in row]
    assert 1.0 in flat
    assert all(torch.equal(r.pred_keypoints.view(torch.int32), b.view(torch.int32)) for r, b in zip(results, before))
