"""GPU suite (pytest -m gpu): the device-side panoptic-quality and semantic confusion kernels
(jtsm_amd/csrc/panoptic_eval.hip) and their evaluators (jtsm_amd/evaluation) against tests/pq_ref.py, the NumPy
restatement that counts pairs with np.unique and the confusion matrix with np.bincount.

tp, fp, fn, the stats words and the confusion matrix must be EQUAL; iou_sum must be BIT-EQUAL to the restatement's
sequential fp64 sum in (image, gt row) order: both sides do one correctly rounded division of the same two integers
per match and then the same ordered adds, so no tolerance is taken.  Shapes are the smallest at which each path can go
wrong: the 4-pixel vector groups and their tail, a map whose address rules the vector loads out, more than one
workgroup, both sides of the LDS bounds."""
import numpy as np
import pytest
import torch

import pq_ref as PR
from test_pq_ref import NUM_CAT, STUFF_CAT, THING_CAT, hand_cases

pytestmark = pytest.mark.gpu

from jtsm_amd.evaluation import panoptic_evaluation as PE  # noqa: E402
from jtsm_amd.evaluation import sem_seg_evaluation as SE  # noqa: E402


def _dev(a, cuda, dtype=torch.int32, misalign=False):
    """Upload; misalign: as a 4-byte-offset view of a larger buffer, so that 16-byte loads are not possible."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    if not misalign:
        return t.to(cuda)
    buf = torch.zeros(t.numel() + 1, dtype=dtype, device=cuda)
    buf[1:] = t.reshape(-1).to(cuda)
    return buf[1:].view(t.shape)


def _device_totals(cuda, images, thing_cat, stuff_cat, C, force_global=False, misalign=False):
    """images: (pred (H,W), pred_table (P,5), num_pred, gt (H,W), gt_table (G,2)) NumPy.  One call per image into fresh
    totals, one read-back at the end."""
    totals = PE.new_totals(C, cuda)
    tc, sc = _dev(np.asarray(thing_cat, np.int32), cuda), _dev(np.asarray(stuff_cat, np.int32), cuda)
    for pred, table, num_pred, gt, gt_table in images:
        out = PE.pq_accumulate(_dev(pred, cuda, misalign=misalign), _dev(np.asarray(table, np.int32).reshape(-1, 5), cuda),
                               torch.full((1,), int(num_pred), dtype=torch.int32, device=cuda), tc, sc,
                               _dev(gt, cuda, misalign=misalign), _dev(np.asarray(gt_table, np.int32).reshape(-1, 2), cuda),
                               totals, force_global=force_global)
        assert out["tables"].is_cuda
    tp, fp, fn, iou_sum, stats = PE.split_totals(totals["tables"].cpu(), C)
    return dict(tp=tp, fp=fp, fn=fn, iou_sum=iou_sum, stats=stats)


def _same(got, want):
    for k in ("tp", "fp", "fn", "stats"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert np.array_equal(got["iou_sum"].view(np.int64), want["iou_sum"].view(np.int64)), (got["iou_sum"], want["iou_sum"])


def _check(cuda, images, thing_cat, stuff_cat, C, **kw):
    got = _device_totals(cuda, images, thing_cat, stuff_cat, C, **kw)
    want = PR.pq_accumulate(images, thing_cat, stuff_cat, C)
    _same(got, want)
    return got


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_worked_cases(cuda, name):
    c = hand_cases()[name]
    image = (c["pred"].reshape(c["shape"]), c["pred_table"], len(c["pred_table"]), c["gt"].reshape(c["shape"]),
             c["gt_table"])
    for kw in ({}, {"force_global": True}):
        got = _check(cuda, [image], THING_CAT, STUFF_CAT, NUM_CAT, **kw)
        assert got["tp"].tolist() == c["tp"] and got["fp"].tolist() == c["fp"] and got["fn"].tolist() == c["fn"]
        want_iou = [0.0, 0.0]
        for cat, num, den in c["iou"]:
            want_iou[cat] += num / den
        assert got["iou_sum"].tolist() == want_iou and got["stats"].tolist() == [0, 0, 0, 1]


# ------------------------------------------------------------------------------------------------ generated images
NUM_GEN_CAT = 8
GEN_THING_CAT, GEN_STUFF_CAT = [0, 1, 2, 3, 4], [5, 6, 7]
GEN_ISTHING = [True] * 5 + [False] * 3


def _generated_image(rng, H, W, rows=3, cols=4, shift=0.3, ids=None):
    """A gt map of rows x cols jittered rectangles (some VOID, some crowd) and a prediction made by shifting every
    rectangle by up to `shift` of its size (later ones paint over earlier ones), mostly with the gt's category."""
    ys = np.linspace(0, H, rows + 1).astype(int)
    xs = np.linspace(0, W, cols + 1).astype(int)
    gt = np.zeros((H, W), np.int32)
    pred = np.zeros((H, W), np.int32)
    gt_table, pred_table = [], []
    for r in range(rows):
        for c in range(cols):
            y0, y1, x0, x1 = ys[r], ys[r + 1], xs[c], xs[c + 1]
            if y1 <= y0 or x1 <= x0 or rng.random() < 0.1:
                continue                                                     # stays VOID
            cat = int(rng.integers(NUM_GEN_CAT))
            gt_table.append([cat, int(rng.random() < 0.12)])
            gt[y0:y1, x0:x1] = len(gt_table)
            if rng.random() < 0.08:
                continue                                                     # no prediction for it
            dy = int(round(rng.uniform(-shift, shift) * (y1 - y0)))
            dx = int(round(rng.uniform(-shift, shift) * (x1 - x0)))
            pcat = cat if rng.random() < 0.85 else int(rng.integers(NUM_GEN_CAT))
            sid = len(pred_table) + 1 if ids is None else int(ids[len(pred_table)])
            region = pred[max(y0 + dy, 0):max(y1 + dy, 0), max(x0 + dx, 0):max(x1 + dx, 0)]
            if region.size == 0:
                continue
            region[...] = sid
            isthing = pcat < 5
            pred_table.append([sid, int(isthing), pcat if isthing else pcat - 5, len(pred_table) if isthing else -1, 0])
    # a painted-over prediction may have lost all its pixels: the reference raises there, so such rows are dropped
    pred_table = [row for row in pred_table if (pred == row[0]).any()]
    return pred, np.array(pred_table, np.int32).reshape(-1, 5), len(pred_table), gt, np.array(gt_table, np.int32).reshape(-1, 2)


@pytest.mark.parametrize("H,W", [(1, 1), (7, 9), (64, 65), (96, 128)])
def test_image_shapes_aligned_and_misaligned(cuda, H, W):
    """1 pixel; 63 = 15 vector groups + a tail of 3; 4160 pixels = two workgroups' worth of groups; 12288.  Each also
    from maps at an address 4 bytes past a 16-byte boundary, which are read pixel by pixel."""
    rng = np.random.default_rng(H * 1000 + W)
    images = [_generated_image(rng, H, W, rows=min(3, H), cols=min(4, W)) for _ in range(3)]
    a = _check(cuda, images, GEN_THING_CAT, GEN_STUFF_CAT, NUM_GEN_CAT)
    b = _check(cuda, images, GEN_THING_CAT, GEN_STUFF_CAT, NUM_GEN_CAT, misalign=True)
    c = _check(cuda, images, GEN_THING_CAT, GEN_STUFF_CAT, NUM_GEN_CAT, force_global=True)
    _same(a, b)
    _same(a, c)
    assert a["stats"].tolist() == [0, 0, 0, 3]


def test_empty_tables(cuda):
    """P = 0 with G > 0 (every gt row a false negative but the crowd), G = 0 with P > 0 (false positives unless on
    VOID — all of it is), both zero."""
    z = np.zeros((5, 6), np.int32)
    gt = z.copy()
    gt[:2] = 1
    gt[2:4] = 2
    got = _check(cuda, [(z, np.zeros((0, 5), np.int32), 0, gt, [[3, 0], [6, 1], [3, 0]])], GEN_THING_CAT, GEN_STUFF_CAT,
                 NUM_GEN_CAT)
    assert got["fn"].tolist() == [0, 0, 0, 2, 0, 0, 0, 0] and got["fp"].sum() == 0
    pred = z.copy()
    pred[1:3] = 9
    got = _check(cuda, [(pred, [[9, 1, 2, 0, 0]], 1, z, np.zeros((0, 2), np.int32))], GEN_THING_CAT, GEN_STUFF_CAT,
                 NUM_GEN_CAT)
    assert got["fp"].sum() == 0 and got["fn"].sum() == 0                       # wholly on VOID: skipped
    got = _check(cuda, [(z, np.zeros((0, 5), np.int32), 0, z, np.zeros((0, 2), np.int32))], GEN_THING_CAT,
                 GEN_STUFF_CAT, NUM_GEN_CAT)
    assert got["stats"].tolist() == [0, 0, 0, 1] and got["tp"].sum() + got["fp"].sum() + got["fn"].sum() == 0


def test_num_pred_smaller_than_the_table_and_non_dense_ids(cuda):
    rng = np.random.default_rng(11)
    ids = [3, 70000, 11, 2 ** 31 - 1, 1 << 20, 77, 12345678, 5, 900, 65536, 65535, 424242]
    pred, table, n, gt, gt_table = _generated_image(rng, 48, 64, ids=ids)
    assert n >= 8 and set(table[:, 0].tolist()) <= set(ids)
    padded = np.concatenate([table, [[4, 1, 0, 0, 0], [6, 0, 1, -1, 0]]]).astype(np.int32)   # rows beyond num_pred
    got = _check(cuda, [(pred, padded, n, gt, gt_table)], GEN_THING_CAT, GEN_STUFF_CAT, NUM_GEN_CAT)
    assert got["stats"].tolist() == [0, 0, 0, 1] and got["tp"].sum() > 0
    # the same table cut short: the pixels of the rows left out name no row
    got = _check(cuda, [(pred, padded, n - 2, gt, gt_table)], GEN_THING_CAT, GEN_STUFF_CAT, NUM_GEN_CAT)
    assert got["stats"][0] == sum(int((pred == sid).sum()) for sid in table[n - 2:, 0]) > 0


def test_stats_words_and_evaluate_raises(cuda):
    """A pixel id in no row, a row without a pixel, a category mapped to -1: each in its own stats word, and each a
    ValueError from evaluate().  The evaluator is fed the dict form of segments_info here."""
    gt_map = np.zeros((4, 6), np.int32)
    gt_map[:, :3] = 1
    base = np.zeros((4, 6), np.int32)
    base[:, :3] = 21
    ok_info = [{"id": 21, "isthing": True, "category_id": 0, "instance_id": 0, "score": 0.9}]
    cases = {
        "pixel": (np.where(np.arange(24).reshape(4, 6) % 6 == 5, 99, base), ok_info, [4, 0, 0]),
        "row": (base, ok_info + [{"id": 22, "isthing": False, "category_id": 0, "area": 7}], [0, 1, 0]),
        "category": (np.where(np.arange(24).reshape(4, 6) % 6 >= 4, 23, base),
                     ok_info + [{"id": 23, "isthing": True, "category_id": 1, "instance_id": 1, "score": 0.5}], [0, 0, 1]),
    }
    for name, (pred, info, want_stats) in cases.items():
        table = [[s["id"], int(s["isthing"]), s["category_id"], s.get("instance_id", -1), s.get("area", 0)] for s in info]
        got = _check(cuda, [(pred.astype(np.int32), table, len(table), gt_map, [[0, 0]])], [0, -1], [1], 2)
        assert got["stats"].tolist() == want_stats + [1], name
        ev = PE.COCOPanopticEvaluator(PE.PanopticGroundTruth.from_arrays(["im"], [gt_map], [[[0, 0]]]), [0, -1], [1],
                                      [True, False], device=cuda)
        ev.process([{"image_id": "im"}], [{"panoptic_seg": (_dev(pred, cuda), info)}])
        with pytest.raises(ValueError, match="panoptic evaluation"):
            ev.evaluate()
        assert ev.last_totals["stats"].tolist() == want_stats + [1], name
    ev = PE.COCOPanopticEvaluator(PE.PanopticGroundTruth.from_arrays(["im"], [gt_map], [[[0, 0]]]), [0, -1], [1],
                                  [True, False], device=cuda)
    ev.process([{"image_id": "im"}], [{"panoptic_seg": (_dev(base, cuda), ok_info)}])
    res = ev.evaluate()["panoptic_seg"]
    assert res["PQ"] == res["PQ_th"] == 100.0 and np.isnan(res["PQ_st"])          # no stuff category was seen
    with pytest.raises(ValueError, match="ground truth"):
        ev.process([{"image_id": "other"}], [{"panoptic_seg": (_dev(base, cuda), ok_info)}])


def _striped(G, P):
    """96 x 128 = 12288 pixels: gt stripes of 96 pixels over the values 0 .. 127, predicted stripes of 96 pixels
    shifted by 16 (IoU 80 / 112 where the categories agree) over 0 .. 127 as non-dense ids."""
    i = np.arange(96 * 128)
    gt = ((i // 96) % 128).astype(np.int32).reshape(96, 128)
    k = ((i + 16) // 96) % 128
    pred = np.where(k == 0, 0, 1000 + 7 * k).astype(np.int32).reshape(96, 128)
    pred_table = [[1000 + 7 * (r + 1), int(r % 3 != 0), r % 3, r, 0] for r in range(P)]
    gt_table = [[(r % 3) if r % 3 else 5 + r % 3, int(r % 17 == 16)] for r in range(G)]
    return pred, np.array(pred_table, np.int32), P, gt, np.array(gt_table, np.int32)


def test_pair_histogram_at_the_lds_bound_and_one_row_above(cuda):
    """(G+1)(P+1) = 128 x 128 = PQ_LDS_CELLS: the LDS form; one gt row more: the global form.  At the bound both forms
    are run on the same input and must give identical totals."""
    assert PE.PQ_LDS_CELLS == 128 * 128
    at = _striped(127, 127)
    lds = _check(cuda, [at], GEN_THING_CAT, GEN_STUFF_CAT, NUM_GEN_CAT)
    glb = _check(cuda, [at], GEN_THING_CAT, GEN_STUFF_CAT, NUM_GEN_CAT, force_global=True)
    _same(lds, glb)
    assert lds["tp"].sum() > 40 and lds["stats"].tolist() == [0, 0, 0, 1]
    above = _check(cuda, [_striped(128, 127)], GEN_THING_CAT, GEN_STUFF_CAT, NUM_GEN_CAT)
    assert above["fn"].sum() == lds["fn"].sum() + 1                               # the new row has no pixel
    assert np.array_equal(above["tp"], lds["tp"]) and np.array_equal(above["iou_sum"], lds["iou_sum"])


def test_forty_generated_images_both_branches_and_bit_reproducible(cuda):
    rng = np.random.default_rng(2024)
    images = []
    for i in range(40):
        H, W = (96, 128) if i not in (7, 23) else ((50, 70) if i == 7 else (33, 200))
        images.append(_generated_image(rng, H, W))
    want = PR.pq_accumulate(images, GEN_THING_CAT, GEN_STUFF_CAT, NUM_GEN_CAT)
    matched, missed = int(want["tp"].sum()), int(want["fn"].sum())
    print("gt rows matched %d, not matched %d; fp %d" % (matched, missed, int(want["fp"].sum())))
    assert matched >= (matched + missed) / 4 and missed >= (matched + missed) / 4
    assert any(im[4][:, 1].any() for im in images)                                # crowds are present
    first = _device_totals(cuda, images, GEN_THING_CAT, GEN_STUFF_CAT, NUM_GEN_CAT)
    again = _device_totals(cuda, images, GEN_THING_CAT, GEN_STUFF_CAT, NUM_GEN_CAT)
    _same(first, want)
    _same(again, first)
    assert first["stats"].tolist() == [0, 0, 0, 40]
    # the evaluator on the same images: the restatement's dictionary
    gt = PE.PanopticGroundTruth.from_arrays(range(40), [im[3] for im in images], [im[4] for im in images])
    ev = PE.COCOPanopticEvaluator(gt, GEN_THING_CAT, GEN_STUFF_CAT, GEN_ISTHING, device=cuda)
    for i, im in enumerate(images):
        info = [{"id": int(r[0]), "isthing": bool(r[1]), "category_id": int(r[2])} for r in im[1]]
        ev.process([{"image_id": i}], [{"panoptic_seg": (_dev(im[0], cuda), info)}])
    assert ev._totals["tables"].is_cuda
    res = ev.evaluate()
    assert res == PR.pq_result_dict(want["tp"], want["fp"], want["fn"], want["iou_sum"], GEN_ISTHING)
    assert 0 < res["panoptic_seg"]["PQ"] < 100


# ------------------------------------------------------------------------------------------------ semantic segmentation
def _device_confusion(cuda, pred, gt, C, ignore, gt_dtype, **kw):
    conf = torch.zeros((C + 1) ** 2 + 1, dtype=torch.int64, device=cuda)
    out = SE.confusion_accumulate(_dev(pred, cuda, torch.int64), _dev(gt, cuda, gt_dtype), C, ignore, conf, **kw)
    assert out.is_cuda
    host = out.cpu().numpy()
    return host[:-1].reshape(C + 1, C + 1), int(host[-1])


@pytest.mark.parametrize("C", [127, 128])
def test_confusion_at_the_lds_bound_and_above(cuda, C):
    """(C+1)^2 = 128^2 = CONFUSION_LDS_CELLS counters in LDS; C = 128: global atomics.  33 x 47 = 1551 pixels: 387
    vector groups and a tail of 3."""
    assert SE.CONFUSION_LDS_CELLS == 128 * 128
    rng = np.random.default_rng(C)
    pred = rng.integers(0, C, (33, 47))
    gt = rng.integers(0, C, (33, 47))
    gt[rng.random((33, 47)) < 0.1] = 255
    pred[:4] = 3                                   # a uniform region: whole wavefronts in one cell
    gt[:4] = 5
    want = PR.confusion(pred, gt, C, 255)
    for dtype in (torch.uint8, torch.int32):
        got, bad = _device_confusion(cuda, pred, gt, C, 255, dtype)
        assert bad == 0 and np.array_equal(got, want)
        if C == 127:
            glb, bad = _device_confusion(cuda, pred, gt, C, 255, dtype, force_global=True)
            assert bad == 0 and np.array_equal(glb, want)


def test_sem_seg_evaluator_matches_bincount(cuda):
    """21 classes at 33 x 47, an ignore label, uint8 and int32 ground truth: the matrix is np.bincount's, the metrics
    are equal as Python floats; two images accumulate."""
    g = torch.Generator().manual_seed(3)
    names = ["c%02d" % i for i in range(21)]
    rng = np.random.default_rng(4)
    logits = [torch.randn(21, 33, 47, generator=g) for _ in range(2)]
    gts = []
    for lg, dt in zip(logits, (np.uint8, np.int32)):
        gt = np.where(rng.random((33, 47)) < 0.6, lg.argmax(dim=0).numpy(), rng.integers(0, 20, (33, 47)))  # class 20 never
        gt[rng.random((33, 47)) < 0.07] = 255
        gts.append(gt.astype(dt))
    ev = SE.SemSegEvaluator(names, 255, {"a": gts[0], "b": gts[1]}, device=cuda)
    ev.process([{"image_id": "a"}, {"image_id": "b"}], [{"sem_seg": lg.to(cuda)} for lg in logits])
    assert ev._conf.is_cuda
    res = ev.evaluate()
    conf = sum(PR.confusion(lg.argmax(dim=0).numpy(), gt, 21, 255) for lg, gt in zip(logits, gts))
    assert np.array_equal(ev.last_conf_matrix, conf) and conf.sum() == 2 * 33 * 47
    want = PR.sem_seg_metrics(conf, names)
    assert list(res["sem_seg"]) == list(want["sem_seg"])
    for k, v in want["sem_seg"].items():
        assert res["sem_seg"][k] == v or (np.isnan(v) and np.isnan(res["sem_seg"][k])), k
    assert 0 < res["sem_seg"]["mIoU"] < 100


def test_sem_seg_out_of_range_raises(cuda):
    """A prediction outside [0, C) (logits of 4 channels against 3 evaluated classes is refused up front; here the
    wrapper gets an arg-max with a 3 in it), and a label that is neither a class nor the ignore label."""
    pred = np.array([[0, 1, 2, 3, 1, 0]])
    got, bad = _device_confusion(cuda, pred, np.zeros((1, 6), np.int64), 3, 255, torch.uint8)
    assert bad == 1 and got.sum() == 5
    ev = SE.SemSegEvaluator(["a", "b", "c"], 255, {"x": np.array([[0, 1, 7, 255, 2, 2]], np.uint8)}, device=cuda)
    ev.process([{"image_id": "x"}], [{"sem_seg": torch.eye(3, 6).view(3, 1, 6).to(cuda)}])
    with pytest.raises(ValueError, match="1 pixels"):
        ev.evaluate()
    with pytest.raises(ValueError, match="channels"):
        ev.process([{"image_id": "x"}], [{"sem_seg": torch.zeros(4, 1, 6).to(cuda)}])


# ------------------------------------------------------------------------------------------------ end to end
def test_evaluators_end_to_end_on_the_panoptic_model(cuda):
    """The small PS_ON model of tests/test_hip_inference.py on two synthetic images, through inference_on_dataset with
    DatasetEvaluators([SemSegEvaluator, COCOPanopticEvaluator]).  Ground truth is made from the model's own outputs:
    image 0 as predicted, image 1 with one segment's category changed and a VOID band.  A third evaluator in the list
    copies the maps of that very pass to the host, and the result must equal the restatement run on those copies."""
    from model_util import jtsm_cfg, to_batched_inputs
    from oracle import model as OM
    from jtsm_amd.evaluation import (COCOPanopticEvaluator, DatasetEvaluator, DatasetEvaluators, PanopticGroundTruth,
                                     SemSegEvaluator, inference_on_dataset)
    from jtsm_amd.modeling import build_model

    torch.manual_seed(0)
    params = OM.init_params(seed=3, random_bn=True, input_gain=1.0 / 64)
    batch = OM.synthetic_batch(1234, B=2, size=256, R=160, sp_block=8)
    cfg = jtsm_cfg("cuda")
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = 1e-5
    cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST = 0.3
    cfg.MODEL.PANOPTIC_FPN.COMBINE.INSTANCES_CONFIDENCE_THRESH = 0.02
    cfg.MODEL.PANOPTIC_FPN.COMBINE.STUFF_AREA_LIMIT = 64
    model = build_model(cfg)
    model.load_state_dict({k: v.detach() for k, v in params.items()}, strict=True)
    model.eval()
    inputs = to_batched_inputs(batch)
    for i, x in enumerate(inputs):
        x["image_id"] = "img%d" % i
    with torch.no_grad():
        outputs = model(inputs)

    num_things, num_stuff = int(cfg.MODEL.ROI_HEADS.NUM_CLASSES), outputs[0]["sem_seg"].shape[0]
    thing_cat, stuff_cat = list(range(num_things)), [num_things + k for k in range(num_stuff)]
    isthing = [True] * num_things + [False] * num_stuff
    C = num_things + num_stuff
    pan_gt, sem_gt = PanopticGroundTruth(), {}
    for i, out in enumerate(outputs):
        pan, info = out["panoptic_seg"]
        assert info.table.is_cuda and info.table.shape == (len(info), 5) and len(info) >= 2
        pan = pan.cpu().numpy()
        dense = np.zeros(pan.shape, np.int32)
        table = []
        for r, s in enumerate(info):
            dense[pan == s["id"]] = r + 1
            table.append([(thing_cat if s["isthing"] else stuff_cat)[s["category_id"]], 0])
        sem = out["sem_seg"].argmax(dim=0).cpu().numpy()
        if i == 0:
            sem = sem.astype(np.uint8)
        else:
            table[0][0] = (table[0][0] + 1) % C                                   # one segment's category changed
            dense[40:60] = 0                                                      # a VOID band
            sem = sem.astype(np.int32)
            sem[40:60] = 255
            sem[100:110] = (sem[100:110] + 1) % num_stuff
        pan_gt.add("img%d" % i, dense, table)
        sem_gt["img%d" % i] = sem

    class Recorder(DatasetEvaluator):
        def reset(self):
            self.seen = []

        def process(self, inputs, outputs):
            for inp, out in zip(inputs, outputs):
                pan, info = out["panoptic_seg"]
                self.seen.append((inp["image_id"], pan.cpu().numpy(), info.table.cpu().numpy(),
                                  out["sem_seg"].argmax(dim=0).cpu().numpy()))

    names = ["s%02d" % k for k in range(num_stuff)]
    sem_ev = SemSegEvaluator(names, 255, sem_gt, device=cuda)
    pan_ev = COCOPanopticEvaluator(pan_gt, thing_cat, stuff_cat, isthing, device=cuda)
    rec = Recorder()
    res = inference_on_dataset(model, [inputs], DatasetEvaluators([sem_ev, pan_ev, rec]))
    assert not model.training and list(res) == ["sem_seg", "panoptic_seg"]
    # the totals stayed on the device until evaluate()'s single copy, and the model's device table was used as it is
    assert sem_ev._conf.is_cuda and pan_ev._totals["tables"].is_cuda
    info = outputs[0]["panoptic_seg"][1]
    assert pan_ev._table_of(info).data_ptr() == info.table.data_ptr()

    images = [(pan, table, len(table)) + tuple(pan_gt[image_id]) for image_id, pan, table, _ in rec.seen]
    want = PR.pq_accumulate(images, thing_cat, stuff_cat, C)
    assert want["stats"].tolist() == [0, 0, 0, 2] and want["tp"].sum() >= 2 and want["fn"].sum() + want["fp"].sum() >= 1
    for k in ("tp", "fp", "fn", "stats"):
        assert np.array_equal(pan_ev.last_totals[k], want[k]), k
    assert np.array_equal(pan_ev.last_totals["iou_sum"].view(np.int64), want["iou_sum"].view(np.int64))
    want_pq = PR.pq_result_dict(want["tp"], want["fp"], want["fn"], want["iou_sum"], isthing)["panoptic_seg"]
    for k, v in want_pq.items():
        assert res["panoptic_seg"][k] == v or (np.isnan(v) and np.isnan(res["panoptic_seg"][k])), k
    conf = sum(PR.confusion(sem, sem_gt[image_id], num_stuff, 255) for image_id, _, _, sem in rec.seen)
    assert np.array_equal(sem_ev.last_conf_matrix, conf)
    want_sem = PR.sem_seg_metrics(conf, names)["sem_seg"]
    for k, v in want_sem.items():
        assert res["sem_seg"][k] == v or (np.isnan(v) and np.isnan(res["sem_seg"][k])), k
    assert res["sem_seg"]["pACC"] > 50
