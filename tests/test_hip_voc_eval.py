"""GPU suite (pytest -m gpu): the device-side Pascal VOC evaluator (jtsm_amd/csrc/voc_eval.hip, jtsm_amd/evaluation)
against tests/voc_eval_ref.py, the NumPy restatement that really prints and parses the detections and ranks with a
stable sort, and against the reference's own recorded outputs (tests/golden/voc_eval_reference.npz).

Bit for bit: `order` (the position of every detection in its class's ranking), `tp_bits` / `fp_bits` (one bit per IoU
threshold 0.50:0.05:0.95), `counts` (npos, npos_im).  As fp64 bit patterns: the 11-point AP and CorLoc tables.  Area AP:
|device - restatement| <= 2 n 2^-53 for a class of n detections — the worst-case reordering error of a sum of n
non-negative terms totalling at most 1 (the reference sums with np.sum, whose pairwise order is not mirrored); derived,
not measured.  Shapes are the smallest at which each loop or rule can go wrong; AP_CHUNK = 256 is voc_eval.hip's
kApChunk, the detections per step of the AP walk."""
import numpy as np
import pytest
import torch

import voc_eval_ref as VR
from conftest import load_cases

pytestmark = pytest.mark.gpu

AP_CHUNK = 256


def _device(cuda, boxes, scores, classes, images, gt, N, C, use_07):
    from jtsm_amd.evaluation import pascal_voc_evaluation as PV

    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(cuda)  # noqa: E731
    gtd = dict(boxes=t(gt[0].reshape(-1, 4), torch.int32), difficult=t(gt[1], torch.uint8), offsets=t(gt[2], torch.int32))
    out = PV.voc_eval(t(np.asarray(boxes, np.float32).reshape(-1, 4), torch.float32), t(np.asarray(scores, np.float32), torch.float32),
                      t(np.asarray(classes), torch.int32), t(np.asarray(images), torch.int32), gtd, N, C, use_07,
                      with_bits=True)
    ap, corloc, stats, counts = PV.split_tables(out["tables"].cpu(), C)
    return dict(ap=ap.copy(), corloc=corloc.copy(), stats=stats.copy(), counts=counts.copy(),
                order=out["order"].cpu().numpy(), tp_bits=out["tp_bits"].cpu().numpy().view(np.uint16),
                fp_bits=out["fp_bits"].cpu().numpy().view(np.uint16))


def _check(cuda, boxes, scores, classes, images, objects, N, C):
    """Both AP forms on the device against the restatement; -> (device result of the 11-point run, restatement)."""
    gt = VR.csr_from_objects(objects, N, C)
    classes = np.asarray(classes)
    n = np.array([(classes == c).sum() for c in range(C)])
    got07 = None
    for use_07 in (True, False):
        got = _device(cuda, boxes, scores, classes, images, gt, N, C, use_07)
        want = VR.evaluate(boxes, scores, classes, images, *gt, N, C, use_07)
        for k in ("order", "tp_bits", "fp_bits", "counts"):
            assert np.array_equal(got[k], want[k]), (k, use_07)
        assert np.array_equal(got["corloc"].view(np.int64), want["corloc"].view(np.int64)), use_07
        if use_07:
            assert np.array_equal(got["ap"].view(np.int64), want["ap"].view(np.int64))
            got07, want07 = got, want
        else:
            err = np.abs(got["ap"] - want["ap"])
            bar = 2.0 * n * 2.0 ** -53
            print("area AP: worst |device - restatement| %.3g, bar %.3g" % (np.nanmax(err, initial=0.0), bar.max()))
            assert np.array_equal(np.isnan(got["ap"]), np.isnan(want["ap"]))
            assert (np.nan_to_num(err) <= bar[None, :]).all(), (err.max(), bar)
        assert got["stats"][2] == 0
        if len(classes):
            s = np.asarray(scores, np.float32)
            assert got["stats"][0] == s.min() and got["stats"][1] == s.max()
    return got07, want07


def _random_case(seed, N, C, dets_per_image, gts_per_image, tie_scores=True):
    rng = np.random.default_rng(seed)
    objects, boxes, scores, classes, images = [], [], [], [], []
    for i in range(N):
        mine = []
        for _ in range(int(rng.integers(0, gts_per_image + 1))):
            x0, y0 = int(rng.integers(1, 300)), int(rng.integers(1, 200))
            o = [i, int(rng.integers(C)), int(rng.random() < 0.2), x0, y0, x0 + int(rng.integers(15, 150)),
                 y0 + int(rng.integers(15, 150))]
            objects.append(o)
            mine.append(o)
        for _ in range(int(rng.integers(0, dets_per_image + 1))):
            if mine and rng.random() < 0.7:
                o = mine[int(rng.integers(len(mine)))]
                wh = np.array([o[5] - o[3], o[6] - o[4]] * 2, float)
                b = np.array([o[3] - 1, o[4] - 1, o[5], o[6]], float) + rng.normal(0, 0.1, 4) * wh
                c = o[1] if rng.random() < 0.9 else int(rng.integers(C))
            else:
                x0, y0 = rng.uniform(0, 300), rng.uniform(0, 200)
                b, c = np.array([x0, y0, x0 + rng.uniform(10, 150), y0 + rng.uniform(10, 150)]), int(rng.integers(C))
            boxes.append(b)
            classes.append(c)
            images.append(i)
            # ties are the normal case with three decimals: a coarse grid makes plenty
            scores.append(rng.integers(1, 200) / 200.0 if tie_scores else rng.random())
    return (np.array(boxes, np.float32).reshape(-1, 4), np.array(scores, np.float32), np.array(classes, np.int32),
            np.array(images, np.int32), np.array(objects, np.int64).reshape(-1, 7))


def test_single_detection(cuda):
    got, _ = _check(cuda, [[9.0, 9.0, 60.0, 60.0]], [0.9], [0], [0], [[0, 0, 0, 10, 10, 60, 60]], 1, 1)
    assert got["tp_bits"][0] == 0x3ff and got["fp_bits"][0] == 0 and got["order"][0] == 0
    assert np.allclose(got["ap"], 1.0, rtol=0, atol=1e-15) and (got["corloc"] == 1.0).all()    # (11 x 1/11 is not 1.0)


@pytest.mark.parametrize("D", [63, 64, 65, AP_CHUNK + 1])
def test_one_class_around_the_wave_and_ap_chunk_sizes(cuda, D):
    """63 / 64 / 65 detections of one class, and AP_CHUNK + 1 = 257: the AP walk's second chunk and its carry."""
    rng = np.random.default_rng(D)
    objects = [[i, 0, int(i % 5 == 4), 10 + i, 20, 90 + i, 120] for i in range(8)]
    boxes, images = [], []
    for k in range(D):
        i = k % 8
        boxes.append(np.array([9 + i, 19, 90 + i, 120], float) + rng.normal(0, 6, 4))
        images.append(i)
    scores = rng.permutation(np.arange(1, 1 + D) / (D + 2.0))
    got, _ = _check(cuda, np.array(boxes, np.float32), scores.astype(np.float32), np.zeros(D, np.int32), images, objects, 8, 1)
    assert 0 < got["ap"][0, 0] < 1


def test_seventy_ground_truth_boxes_in_one_image(cuda):
    """The second lane chunk of the match and a claimed set beyond 64: boxes 64..69 are matched, and box 66 twice."""
    G = 70
    objects = [[0, 0, int(j == 65), 1 + 12 * j, 5, 10 + 12 * j, 40] for j in range(G)]
    js = [69, 66, 3, 66, 64, 65, 0, 63, 67, 68, 64]
    boxes = [[12.0 * j + 0.2 * (k % 3), 4.0, 10.0 + 12 * j, 40.0 + 0.3 * (k % 2)] for k, j in enumerate(js)]
    scores = [0.95 - 0.05 * k for k in range(len(js))]
    got, _ = _check(cuda, boxes, scores, np.zeros(len(js), np.int32), np.zeros(len(js), np.int32), objects, 1, 1)
    assert got["tp_bits"][1] & 1 and got["fp_bits"][3] & 1            # box 66: claimed, then taken
    assert got["tp_bits"][4] & 1 and got["fp_bits"][10] & 1           # box 64 likewise
    assert got["tp_bits"][5] == 0 and got["fp_bits"][5] & 1 == 0      # box 65 is difficult: neither


def test_image_without_ground_truth_all_difficult_and_five_on_one_box(cuda):
    objects = [[1, 0, 1, 10, 10, 80, 80], [1, 0, 1, 100, 10, 180, 80],           # image 1: all difficult
               [2, 0, 0, 20, 20, 120, 140]]                                       # image 2: five detections on it
    boxes = [[5, 5, 70, 70], [9, 9, 80, 80], [99, 9, 180, 80]] + [[19 + 0.3 * k, 19, 120, 140 - 0.4 * k] for k in range(5)]
    images = [0, 1, 1, 2, 2, 2, 2, 2]
    scores = [0.99, 0.9, 0.8, 0.7, 0.65, 0.6, 0.55, 0.5]
    got, _ = _check(cuda, boxes, scores, np.zeros(8, np.int32), images, objects, 3, 1)
    assert got["fp_bits"][0] == 0x3ff and got["tp_bits"][0] == 0                  # no ground truth in image 0
    assert (got["tp_bits"][1:3] == 0).all() and (got["fp_bits"][1:3] == 0).all()  # difficult: neither
    assert [int(b & 1) for b in got["tp_bits"][3:]] == [1, 0, 0, 0, 0]
    assert [int(b & 1) for b in got["fp_bits"][3:]] == [0, 1, 1, 1, 1]
    assert got["counts"].tolist() == [[1, 1]]
    assert got["corloc"][0, 0] == 1.0                                            # only image 2 counts


def test_iou_exactly_on_a_threshold_is_not_above_it(cuda):
    """Integer boxes: 100 / 200 = 0.5 and 300 / 400 = 0.75 exactly, and `>` is strict."""
    objects = [[0, 0, 0, 1, 1, 10, 10], [1, 0, 0, 1, 1, 20, 20]]
    boxes = [[0, 0, 10, 20], [0, 0, 20, 15]]
    got, _ = _check(cuda, boxes, [0.9, 0.8], [0, 0], [0, 1], objects, 2, 1)
    assert got["tp_bits"][0] == 0 and got["fp_bits"][0] == 0x3ff
    assert got["tp_bits"][1] == 0b0000011111 and got["fp_bits"][1] == 0b1111100000


def test_equal_overlaps_take_the_first_maximum(cuda):
    """Two identical ground-truth boxes: both detections pick the first, so the second is a false positive although
    the other box is free — np.argmax's first maximum.  With the first one difficult both are ignored."""
    for diff, tp, fp in ((0, [1, 0], [0, 1]), (1, [0, 0], [0, 0])):
        objects = [[0, 0, diff, 10, 10, 60, 60], [0, 0, 0, 10, 10, 60, 60]]
        got, _ = _check(cuda, [[9, 9, 60, 60], [9, 9, 60, 60]], [0.9, 0.8], [0, 0], [0, 0], objects, 1, 1)
        assert [int(b & 1) for b in got["tp_bits"]] == tp and [int(b & 1) for b in got["fp_bits"]] == fp


def test_quantisation_half_way_cases(cuda):
    """Half to even on the exact binary value, as Python's formatting: 0.0625 -> 0.062 ranks BELOW 0.063, 0.1875 -> 0.188
    ties with 0.188; ymax 1.25 -> 1.2 and 1.75 -> 1.8 against a box of height 2 (IoU = ymax / 2: a tenth is a threshold
    step); xmin = 0.25 + 2^-25, whose fp32 `+ 1` rounds to 1.25 -> 1.2 (in double it would print 1.3)."""
    objects = [[i, 0, 0, 1, 1, 10, 2] for i in range(2)] + [[2, 0, 0, 1, 1, 2, 10]] + [[3, 0, 0, 1, 1, 50, 50]]
    x = np.float32(0.25) + np.float32(2.0 ** -25)
    assert float(x) > 0.25 and np.float32(x + np.float32(1)) == np.float32(1.25)
    boxes = np.array([[0, 0, 10, 1.25], [0, 0, 10, 1.75], [x, 0, 2, 10], [0, 0, 50, 50], [0, 0, 50, 50], [0, 0, 50, 50]],
                     np.float32)
    scores = np.array([0.9, 0.8, 0.7, 0.0625, 0.063, 0.1875], np.float32)
    got, _ = _check(cuda, boxes, scores, np.zeros(6, np.int32), [0, 1, 2, 3, 3, 3], objects, 4, 1)
    assert got["tp_bits"][0] == 0b0000000011          # IoU 0.6: above 0.50 and 0.55, not above 0.60
    assert got["tp_bits"][1] == 0b0011111111          # IoU 0.9: above 0.50 .. 0.85
    assert got["tp_bits"][2] == 0b0011111111          # xmin prints 1.2: IoU 0.9 (1.3 would give 0.85: seven bits)
    assert got["order"].tolist() == [0, 1, 2, 5, 4, 3]


def test_equal_quantised_scores_rank_in_arrival_order(cuda):
    """Across images and within one image.  0.5004 and 0.4996 both print 0.500: arrival order decides who claims."""
    objects = [[0, 0, 0, 10, 10, 60, 60], [1, 0, 0, 10, 10, 60, 60]]
    boxes = [[9, 9, 60, 60.4], [9, 9, 60, 60], [9, 9, 60, 60], [9.2, 9, 60, 60]]
    got, _ = _check(cuda, boxes, [0.4996, 0.5004, 0.5, 0.5001], [0, 0, 0, 0], [1, 0, 1, 0], objects, 2, 1)
    assert got["order"].tolist() == [0, 1, 2, 3]
    assert [int(b & 1) for b in got["tp_bits"]] == [1, 1, 0, 0]


def test_class_without_detections_and_class_without_ground_truth(cuda):
    """Class 1 has ground truth and no detection: 0.  Class 2 has detections and no ground truth: 11-point AP 0, area
    AP NaN, CorLoc NaN (the reference divides by zero; evaluate() raises)."""
    objects = [[0, 0, 0, 10, 10, 60, 60], [0, 1, 0, 10, 10, 60, 60]]
    got, _ = _check(cuda, [[9, 9, 60, 60], [9, 9, 60, 60]], [0.9, 0.8], [0, 2], [0, 0], objects, 1, 3)
    assert (got["ap"][:, 1] == 0).all() and (got["corloc"][:, 1] == 0).all()
    assert (got["ap"][:, 2] == 0).all() and np.isnan(got["corloc"][:, 2]).all()
    assert got["counts"].tolist() == [[1, 1], [1, 1], [0, 0]]


def test_random_200_images_20_classes(cuda):
    boxes, scores, classes, images, objects = _random_case(5, 200, 20, 30, 5)
    got, _ = _check(cuda, boxes, scores, classes, images, objects, 200, 20)
    assert 0 < np.nanmean(got["ap"][0]) < 1 and len(scores) > 2000


def test_out_of_range_indices_are_left_out_and_reported(cuda):
    gt = VR.csr_from_objects([[0, 0, 0, 10, 10, 60, 60]], 1, 1)
    got = _device(cuda, [[9, 9, 60, 60]] * 3, [0.9, 0.8, 0.7], [0, 1, -1], [0, 0, 0], gt, 1, 1, True)
    assert got["stats"][2] == 2 and got["order"].tolist() == [0, -1, -1] and abs(got["ap"][0, 0] - 1.0) < 1e-15


def test_golden_cases_match_the_reference_on_the_device(cuda):
    """The reference's own recorded numbers (no equal quantised scores inside a class): 11-point AP and CorLoc equal,
    area AP within the bar."""
    for name, z in load_cases("voc_eval_reference.npz").items():
        N, C = int(z["num_images"]), z["ap07"].shape[1]
        gt = VR.csr_from_objects(z["objects"], N, C)
        args = (z["det_boxes"], z["det_scores"], z["det_classes"], z["det_images"], gt, N, C)
        a, b = _device(cuda, *args, True), _device(cuda, *args, False)
        assert np.array_equal(a["ap"].view(np.int64), z["ap07"].view(np.int64)), name
        assert np.array_equal(a["corloc"], z["corloc"], equal_nan=True), name
        n = np.array([(z["det_classes"] == c).sum() for c in range(C)])
        assert np.array_equal(np.isnan(b["ap"]), np.isnan(z["ap12"])), name
        assert (np.nan_to_num(np.abs(b["ap"] - z["ap12"])) <= 2.0 * n[None, :] * 2.0 ** -53).all(), name
        # the TP / FP bits give the recorded precision / recall curves
        lo = 0
        for c in range(C):
            idx = np.nonzero(z["det_classes"] == c)[0]
            ranked = idx[np.argsort(a["order"][idx])]
            for t in range(10):
                tp = np.cumsum((a["tp_bits"][ranked] >> t) & 1).astype(float)
                fp = np.cumsum((a["fp_bits"][ranked] >> t) & 1).astype(float)
                with np.errstate(divide="ignore", invalid="ignore"):
                    rec = tp / float(a["counts"][c, 0])
                assert np.array_equal(rec, z["rec"][t, lo:lo + len(idx)], equal_nan=True), (name, c, t)
                assert np.array_equal(tp / np.maximum(tp + fp, np.finfo(np.float64).eps), z["prec"][t, lo:lo + len(idx)])
            lo += len(idx)


def test_evaluator_end_to_end_on_oicr_mist_detections(cuda):
    """The OICR + MIST model of tests/test_hip_oicr_model.py (same flattened shipped config and size) infers two
    synthetic images; process() keeps the detections on the device; evaluate()'s dictionary equals the restatement's
    on the same detections copied to the host; a second evaluate() gives the same bits."""
    from model_util import to_batched_inputs
    from test_hip_oicr_model import _batch, _model, _params
    from jtsm_amd.evaluation import DatasetEvaluator, PascalVOCDetectionEvaluator, VOCGroundTruth, inference_on_dataset

    batch = _batch(R=200)
    model = _model(_params())
    model.roi_heads.box_refinery[-1].test_score_thresh = 1e-5
    model.roi_heads.box_refinery[-1].test_nms_thresh = 0.3
    model.eval()
    inputs = to_batched_inputs(batch)
    for i, x in enumerate(inputs):
        x["image_id"] = "img%d" % i
    with torch.no_grad():
        outputs = model(inputs)
    host = [(o["instances"].pred_boxes.tensor.cpu().numpy(), o["instances"].scores.cpu().numpy(),
             o["instances"].pred_classes.cpu().numpy()) for o in outputs]
    assert all(len(h[1]) > 0 for h in host)
    # synthetic ground truth: per image and class the best detection's box in integers (some more, some difficult)
    dicts = []
    for i, (b, s, c) in enumerate(host):
        annos = []
        for k in np.unique(c):
            rows = np.nonzero(c == k)[0]
            for r, row in enumerate(rows[np.argsort(-s[rows], kind="stable")][:2]):
                x0, y0, x1, y1 = np.round(b[row]).astype(int)
                annos.append({"category_id": int(k), "bbox": [float(x0), float(y0), float(max(x1, x0 + 2)), float(max(y1, y0 + 2))],
                              "difficult": int(r == 1 and k % 3 == 0)})
        dicts.append({"image_id": "img%d" % i, "annotations": annos})
    names = ["c%02d" % k for k in range(20)]
    gt = VOCGroundTruth.from_dataset_dicts(dicts, 20)
    # every class must have an image with a non-difficult box, or CorLoc is undefined: give absent classes one
    present = set(a["category_id"] for d in dicts for a in d["annotations"])
    for k in range(20):
        if k not in present:
            dicts[0]["annotations"].append({"category_id": k, "bbox": [3.0, 3.0, 30.0, 30.0]})
    gt = VOCGroundTruth.from_dataset_dicts(dicts, 20)
    ev = PascalVOCDetectionEvaluator(names, gt, 2007, device=cuda)
    assert isinstance(ev, DatasetEvaluator)
    ev.reset()
    ev.process(inputs, outputs)
    stored = ev._boxes + ev._scores + ev._classes
    assert len(stored) == 6 and all(t.is_cuda for t in stored)
    assert ev._boxes[0].data_ptr() == outputs[0]["instances"].pred_boxes.tensor.data_ptr()     # a reference, not a copy
    res = ev.evaluate()
    want = VR.evaluate(np.concatenate([h[0] for h in host]), np.concatenate([h[1] for h in host]),
                       np.concatenate([h[2] for h in host]),
                       np.concatenate([np.full(len(h[1]), i) for i, h in enumerate(host)]),
                       gt.gt_boxes, gt.gt_difficult, gt.gt_offsets, 2, 20, True)
    want = VR.result_dict(want["ap"], want["corloc"])
    assert set(res) == {"bbox", "bbox CorLoc"}
    for grp in want:
        for k, v in want[grp].items():
            assert res[grp][k] == v, (grp, k, res[grp][k], v)
    assert res["bbox"]["AP50"] > 0 and res["bbox CorLoc"]["CL50"] > 0
    first = {k: ev.last_tables[k].copy() for k in ("ap", "corloc", "counts")}
    again = ev.evaluate()
    assert again == res
    for k, v in first.items():
        assert np.array_equal(v.view(np.int64) if v.dtype == np.float64 else v,
                              ev.last_tables[k].view(np.int64) if v.dtype == np.float64 else ev.last_tables[k]), k
    # the loop itself, and the empty evaluator
    res2 = inference_on_dataset(model, [inputs], ev)
    assert res2 == res and not model.training
    ev.reset()
    zero = ev.evaluate()
    assert all(v == 0 for grp in zero.values() for v in grp.values())
    with pytest.raises(ValueError):
        ev.process([{"image_id": "nope"}], outputs[:1])


def test_evaluate_refuses_scores_outside_the_unit_interval_and_undefined_corloc(cuda):
    from jtsm_amd.evaluation import PascalVOCDetectionEvaluator, VOCGroundTruth
    from jtsm_amd.structures import Boxes, Instances

    gt = VOCGroundTruth(["a"], [[0, 0, 0, 10, 10, 60, 60]], 2)

    def run(score, cls):
        ev = PascalVOCDetectionEvaluator(["x", "y"], gt, 2012, device=cuda)
        inst = Instances((100, 100), pred_boxes=Boxes(torch.tensor([[9.0, 9.0, 60.0, 60.0]], device=cuda)),
                         scores=torch.tensor([score], device=cuda), pred_classes=torch.tensor([cls], device=cuda))
        ev.process([{"image_id": "a"}], [{"instances": inst}])
        return ev.evaluate()

    assert run(0.5, 0)["bbox"]["AP50"] == 50.0                       # class x: 100, class y: 0
    with pytest.raises(ValueError, match="0, 1"):
        run(1.5, 0)
    with pytest.raises(ValueError, match="y"):
        run(0.5, 1)
    with pytest.raises(ValueError, match="class"):
        run(0.5, 2)
