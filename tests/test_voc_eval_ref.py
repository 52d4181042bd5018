"""CPU suite: the NumPy restatement of the Pascal VOC evaluation (tests/voc_eval_ref.py) against the reference's own
outputs recorded in tests/golden/voc_eval_reference.npz (tests/golden/make_voc_eval_golden.py: cases without equal
quantised scores inside a class, where the reference does not hang on its unstable sort), the ground-truth
constructors, and the host side of the jtsm_voc_eval entry point (no GPU is touched)."""
import ctypes as C
import os

import numpy as np
import pytest

import voc_eval_ref as VR
from conftest import load_cases

NAMES = ["aeroplane", "bicycle", "bird", "boat", "bottle", "bus"]


@pytest.fixture(scope="module")
def golden():
    return load_cases("voc_eval_reference.npz")


@pytest.fixture(scope="module")
def restated(golden):
    """{case: {use_07: result of the restatement}} — computed once."""
    out = {}
    for name, z in golden.items():
        N = int(z["num_images"])
        gt = VR.csr_from_objects(z["objects"], N, len(NAMES))
        out[name] = {m: VR.evaluate(z["det_boxes"], z["det_scores"], z["det_classes"], z["det_images"], *gt, N,
                                    len(NAMES), m, keep_curves=True) for m in (True, False)}
    return out


def test_golden_cases_cover_what_they_must(golden):
    assert len(golden) >= 3
    seen = dict(difficult=False, class_without_gt_with_dets=False, class_without_dets=False, only_difficult=False,
                result=False)
    for z in golden.values():
        o, cls = z["objects"], z["det_classes"]
        seen["difficult"] |= bool(o[:, 2].any())
        for c in range(len(NAMES)):
            has_gt, has_det = bool((o[:, 1] == c).any()), bool((cls == c).any())
            seen["class_without_gt_with_dets"] |= (not has_gt) and has_det
            seen["class_without_dets"] |= has_gt and not has_det
            for i in range(int(z["num_images"])):
                d = o[(o[:, 0] == i) & (o[:, 1] == c), 2]
                seen["only_difficult"] |= len(d) > 0 and bool(d.all())
        seen["result"] |= "result2007" in z and "result2012" in z
        conf, _ = VR.through_text(z["det_boxes"], z["det_scores"])
        for c in range(len(NAMES)):
            v = conf[cls == c]
            assert len(np.unique(v)) == len(v)                      # the condition the recording stands on
    assert all(seen.values()), seen


def test_restatement_reproduces_the_reference(golden, restated):
    """rec / prec (from TP / FP), the 11-point AP and CorLoc equal; area AP within 2 n 2^-53 (np.sum's pairwise order
    over the same terms is the restatement's too, so it is equal in practice — the bound is the device test's)."""
    for name, z in golden.items():
        got07, got12 = restated[name][True], restated[name][False]
        Cn = len(NAMES)
        for t in range(10):
            rec = np.concatenate([got07["curves"][(t, c)][0] for c in range(Cn)])
            prec = np.concatenate([got07["curves"][(t, c)][1] for c in range(Cn)])
            assert np.array_equal(rec, z["rec"][t], equal_nan=True), (name, t)
            assert np.array_equal(prec, z["prec"][t], equal_nan=True), (name, t)
        assert np.array_equal(got07["ap"].view(np.int64), z["ap07"].view(np.int64)), name
        assert np.array_equal(got07["corloc"], z["corloc"], equal_nan=True), name
        assert np.array_equal(got12["corloc"], z["corloc"], equal_nan=True), name
        n = np.array([(z["det_classes"] == c).sum() for c in range(Cn)])
        bar = 2.0 * n * 2.0 ** -53
        assert np.array_equal(np.isnan(got12["ap"]), np.isnan(z["ap12"])), name
        assert (np.nan_to_num(np.abs(got12["ap"] - z["ap12"])) <= bar[None, :]).all(), name
        for year, got in ((2007, got07), (2012, got12)):
            key = "result%d" % year
            if key in z:
                r = VR.result_dict(got["ap"], got["corloc"])
                mine = np.array([r["bbox"][k] for k in ("AP", "AP50", "AP75")]
                                + [r["bbox CorLoc"][k] for k in ("CL", "CL50", "CL75")])
                if year == 2007:
                    assert np.array_equal(mine, z[key]), (name, year)
                else:
                    assert np.allclose(mine, z[key], rtol=0, atol=100 * bar.max()), (name, year)


def test_quantisation_through_text():
    conf, bb = VR.through_text([[2.25, 2.75, 11.25, 11.75], [16777216.0, 0.04999, 2.0, 3.0]], [0.0625, 0.1875])
    assert conf.tolist() == [0.062, 0.188]
    assert bb[0].tolist() == [3.2, 3.8, 11.2, 11.8]                 # half to even on the exact binary value
    assert bb[1, 0] == 16777216.0                                   # the fp32 `+ 1` rounds back: 2^24 + 1 is no fp32
    assert bb[1, 1] == 1.0                                          # fp32(0.04999 + 1) prints 1.0


def _write_tree(tmp, objects, N):
    ids = ["%06d" % (i + 1) for i in range(N)]
    os.makedirs(os.path.join(tmp, "Annotations"))
    with open(os.path.join(tmp, "test.txt"), "w") as f:
        f.write("\n".join(ids) + "\n")
    for i, name in enumerate(ids):
        body = "".join(
            "<object><name>%s</name><pose>Left</pose><truncated>1</truncated><difficult>%d</difficult><bndbox>"
            "<xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>"
            % ((NAMES + ["sofa"])[o[1]], o[2], o[3], o[4], o[5], o[6]) for o in objects if o[0] == i)
        with open(os.path.join(tmp, "Annotations", name + ".xml"), "w") as f:
            f.write("<annotation>%s</annotation>" % body)
    return ids


def test_both_constructors_give_the_same_sorted_arrays_and_csr(golden, tmp_path):
    from jtsm_amd.evaluation import VOCGroundTruth

    z = golden["case0"]
    N, objects = int(z["num_images"]), z["objects"]
    extra = np.concatenate([objects, [[2, len(NAMES), 0, 5, 5, 50, 50]]])        # a class that is not evaluated
    ids = _write_tree(str(tmp_path), extra, N)
    a = VOCGroundTruth.from_voc_xml(os.path.join(str(tmp_path), "Annotations"), os.path.join(str(tmp_path), "test.txt"),
                                    NAMES)
    dicts = [{"image_id": ids[i],
              "annotations": [{"category_id": int(o[1]), "bbox": [float(o[3]) - 1.0, float(o[4]) - 1.0, float(o[5]),
                                                                  float(o[6])], "bbox_mode": 0,
                               **({"difficult": 1} if o[2] else {})} for o in objects if o[0] == i]}
             for i in range(N)]
    b = VOCGroundTruth.from_dataset_dicts(dicts, len(NAMES))
    want = VR.csr_from_objects(objects, N, len(NAMES))
    for g in (a, b):
        assert g.image_ids == ids and g.num_images == N and g.num_classes == len(NAMES)
        assert g.gt_boxes.dtype == np.int32 and g.gt_difficult.dtype == np.uint8 and g.gt_offsets.dtype == np.int32
        assert np.array_equal(g.gt_boxes, want[0]) and np.array_equal(g.gt_difficult, want[1])
        assert np.array_equal(g.gt_offsets, want[2])


def test_workspace_query_is_monotone_and_nonzero_for_no_detections():
    from jtsm_amd import _lib

    lib = _lib.lib()

    def q(d, g, c):
        return lib.jtsm_voc_eval_workspace_bytes(d, g, c)

    assert q(0, 0, 1) > 0 and q(0, 0, 20) > 0                       # D = 0: no division by zero, something to align
    sizes = [0, 1, 63, 64, 65, 257, 4096, 100000, 495200, 5000000]
    last = 0
    for d in sizes:
        v = q(d, 1000, 20)
        assert v >= last, (d, v, last)
        last = v
    assert q(1000, 0, 20) <= q(1000, 5000, 20) <= q(1000, 500000, 20)
    assert q(1000, 100, 1) <= q(1000, 100, 20) <= q(1000, 100, 2000)
    assert q(495200, 15000, 20) >= 495200 * (8 * 4 + 4 * 3 + 32)     # keys, indices and quantised boxes at least


def test_entry_point_refuses_sizes_beyond_the_key_bits():
    """C and N are checked on the host before anything is launched: no GPU is needed to be refused."""
    from jtsm_amd import _lib

    lib = _lib.lib()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)

    def call(N, Cn):
        return lib.jtsm_voc_eval(None, None, None, None, 0, None, None, p, 0, N, Cn, 1, p, p, p, p, None, None, None,
                                 p, 1 << 20, None)

    assert call(4952, 1 << 16) == -1
    assert b"class bits" in lib.jtsm_last_error()
    assert call((1 << 24) + 1, 20) == -1
    assert b"image bits" in lib.jtsm_last_error()
    assert call(0, 20) == -1 and call(10, 0) == -1
