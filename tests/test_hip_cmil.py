"""GPU suite (pytest -m gpu): roi_merge and roi_label (jtsm_amd/csrc/cmil.hip) against the NumPy restatement of
ROIMerge_cpu.cpp and ROILabel_cpu.cpp (tests/cmil_ref.py), bit for bit.

Row counts per image cover one row, one short window (39), a window and a row (41), the top-200 boundary (199, 201),
a ragged batch (300, 7), the training shape (2000, 1500) and more than 8 x 1024 rows (8300: a ninth ranking workgroup,
a ninth chunk of ROILabel's scan).  ROIMerge runs at lam 0, 0.3, 0.6 and 1 with 3 and 20 classes; compared are I, IC,
merged_offsets, MC and MD on the live rows (the dead rows must be zero) and the backward's dC, dD for a random
upstream.  ROILabel runs with 1-6 present classes in three modes: raw scores with the image probabilities as weights,
raw scores with the seeds' scores as weights (both: everything bit-equal), and logits + lse (the seeds' rows are
asserted equal first — the device's expf against NumPy's exp decides them — then labels and weights bit for bit).

The generator (cmil_ref.merge_case / label_case) piles the boxes on 4 rectangles and asserts that the scores have no
ties and that no compared IoU lies within 1e-6 of lam or of a threshold (exact 0 and 1 apart); it may discard at most
half of the seeds it tries."""
import numpy as np
import pytest
import torch

import cmil_ref as CR

pytestmark = pytest.mark.gpu

ROWS = [[1], [39], [41], [199, 201], [300, 7], [2000, 1500], [8300]]
PRESENT = {(1,): 3, (39,): 1, (41,): 2, (199, 201): 4, (300, 7): 5, (2000, 1500): 6, (8300,): 2}
LAMS = [0.0, 0.3, 0.6, 1.0]
MODES = ["raw", "raw_seed_weight", "logits"]
IDS = ["-".join(map(str, r)) for r in ROWS]
FG, BG_HI, BG_LO = 0.6, 0.4, 0.1


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda", 0)


def _generate(make):
    """The first of at most two seeds whose case is well defined."""
    for tried, seed in enumerate((1, 2), 1):
        case = make(seed)
        if case is not None:
            return case
    raise AssertionError("the generator discarded %d of %d seeds" % (tried, tried))


_MERGE = {}


def _merge_reference(rows, K, lam):
    key = (tuple(rows), K, lam)
    if key not in _MERGE:
        case = _generate(lambda seed: CR.merge_case(seed * 100 + len(rows), rows, K, lam))
        _MERGE[key] = (case, CR.roi_merge(case["S"], case["boxes"], case["C"], case["D"], case["offsets"], case["lam"]))
    return _MERGE[key]


@pytest.mark.parametrize("K", [3, 20])
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("rows", ROWS, ids=IDS)
def test_roi_merge_matches_the_restatement(cuda, rows, lam, K):
    from jtsm_amd.layers.cmil import roi_merge

    case, want = _merge_reference(rows, K, lam)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    C, D = t(case["C"]).requires_grad_(True), t(case["D"]).requires_grad_(True)
    MC, MD, I, IC, moff = roi_merge(t(case["S"]), t(case["boxes"]), C, D, t(case["offsets"]), float(case["lam"]), max(rows))
    assert I.dtype == IC.dtype == moff.dtype == torch.int32 and moff.is_cuda
    assert not I.requires_grad and MC.requires_grad and MD.requires_grad
    assert np.array_equal(moff.cpu().numpy(), want["merged_offsets"])
    assert np.array_equal(I.cpu().numpy(), want["I"])
    assert np.array_equal(IC.cpu().numpy(), want["IC"])
    live = int(want["merged_offsets"][-1])
    for name, got in (("MC", MC), ("MD", MD)):
        got = got.detach().cpu().numpy()
        assert np.array_equal(got[:live], want[name][:live]), name
        assert not got[live:].any(), name                                          # dead rows
    g = torch.Generator().manual_seed(3)
    gMC, gMD = torch.randn(MC.shape, generator=g), torch.randn(MC.shape, generator=g)
    ((MC * gMC.to(cuda)).sum() + (MD * gMD.to(cuda)).sum()).backward()
    wC, wD = CR.roi_merge_backward(gMC.numpy(), gMD.numpy(), want["I"], want["IC"])
    assert np.array_equal(C.grad.cpu().numpy(), wC) and np.array_equal(D.grad.cpu().numpy(), wD)


def test_roi_merge_clique_sizes_span_one_to_forty():
    sizes = set()
    for lam in LAMS:
        _, want = _merge_reference([2000, 1500], 3, lam)
        live = int(want["merged_offsets"][-1])
        sizes |= set(want["IC"][:live].tolist())
        assert want["IC"][live:].sum() == 0 and want["IC"][:live].sum() == 3500
    assert min(sizes) == 1 and max(sizes) == 40, sorted(sizes)


def test_roi_merge_takes_strided_logits(cuda):
    """C and D as column slices of one wider GEMM output, each with its own leading dimension."""
    from jtsm_amd.layers.cmil import roi_merge

    case, want = _merge_reference([300, 7], 3, 0.3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    wide = torch.zeros(307, 11, device=cuda)
    wide[:, 2:5] = t(case["C"])
    Dw = torch.zeros(307, 7, device=cuda)
    Dw[:, 4:7] = t(case["D"])
    MC, MD, I, _, _ = roi_merge(t(case["S"]), t(case["boxes"]), wide[:, 2:5], Dw[:, 4:7], t(case["offsets"]), 0.3, 300)
    assert np.array_equal(I.cpu().numpy(), want["I"])
    assert np.array_equal(MC.cpu().numpy(), want["MC"]) and np.array_equal(MD.cpu().numpy(), want["MD"])


# ---- ROILabel ------------------------------------------------------------------------------------------------------------
def _scores(case):
    """The class scores as the reference's S holds them: raw, or the soft-max of the logits (predict_probs)."""
    if case["mode"] == "raw":
        return case["S"]
    z = torch.from_numpy(case["S"])
    return torch.softmax(z, dim=1).numpy()


def _label_well_defined(case, want):
    for b, w in enumerate(want):
        lo, hi = case["offsets"][b], case["offsets"][b + 1]
        if not w["seed_rows"]:
            continue
        bx = case["boxes"][lo:hi]
        sb = bx[w["seed_rows"]]
        if not CR.far_from(CR.pairwise_iou(bx, sb), bx, sb, [FG, BG_HI, BG_LO]):
            return False
    return True


_LABEL = {}


def _label_reference(rows, mode):
    key = (tuple(rows), mode)
    if key not in _LABEL:
        def make(seed):
            case = CR.label_case(seed * 100 + len(rows), rows, PRESENT[tuple(rows)], mode="raw" if mode != "logits" else "logits")
            if case is None:
                return None
            S = _scores(case)
            want = []
            for b in range(len(rows)):
                lo, hi = case["offsets"][b], case["offsets"][b + 1]
                ids = case["classes"][b, :case["counts"][b]]
                want.append(CR.roi_label_image(S[lo:hi], case["boxes"][lo:hi], ids,
                                               case["CW"][b] if mode != "raw_seed_weight" else None, case["perm"][lo:hi],
                                               FG, BG_HI, BG_LO, 32, 96, 1, num_classes=case["K"]))
            return (case, want) if _label_well_defined(case, want) else None
        _LABEL[key] = _generate(make)
    return _LABEL[key]


def _device_label(case, mode, cuda, perm="case", generator=None):
    from jtsm_amd.layers.cmil import roi_label
    from jtsm_amd.layers.mining import row_lse

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    S = t(case["S"])
    return roi_label(S, t(case["boxes"]), t(case["offsets"]), t(case["classes"]), t(case["counts"]),
                     t(case["CW"]) if mode != "raw_seed_weight" else None, rows_per_image=case["rows"],
                     perm=t(case["perm"]) if perm == "case" else perm, generator=generator,
                     lse=row_lse(S) if mode == "logits" else None, fg=FG, bg_hi=BG_HI, bg_lo=BG_LO, num_pos=32, num_neg=96,
                     top_k=1, num_classes=case["K"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows", ROWS, ids=IDS)
def test_roi_label_matches_the_restatement(cuda, rows, mode):
    case, want = _label_reference(rows, mode)
    out = _device_label(case, mode, cuda)
    seeds, num = out["seed_rows"].cpu().numpy(), out["seed_num"].cpu().numpy()
    labels, weights = out["labels"].cpu().numpy(), out["weights"].cpu().numpy()
    for b, w in enumerate(want):
        lo, hi = case["offsets"][b], case["offsets"][b + 1]
        k = len(w["seed_rows"])
        assert int(num[b]) == k and seeds[b, :k].tolist() == w["seed_rows"], b       # the seeds first
        assert (seeds[b, k:] == -1).all()
        assert np.array_equal(labels[lo:hi], w["labels"]), b
        assert np.array_equal(weights[lo:hi], w["weights"]), b                       # (CW or a raw score: no arithmetic)


def test_roi_label_cases_cover_binding_and_idle_caps_and_classes_beyond_rows():
    binds = {}
    for rows in ROWS:
        case, want = _label_reference(rows, "raw")
        for b, w in enumerate(want):
            binds[(tuple(rows), b)] = (w["eligible"][0] > 33, w["eligible"][1] > 97)
            if w["eligible"][0] > 33:
                assert int((w["weights"][w["labels"] < case["K"]] > 0).sum()) == 33
            if w["eligible"][1] > 97:
                assert int((w["labels"] == case["K"]).sum()) == 97
    assert binds[((2000, 1500), 0)] == (True, True) and binds[((8300,), 0)] == (True, True), binds
    assert any(v == (False, False) for v in binds.values()), binds
    case, want = _label_reference([1], "raw")
    assert int(case["counts"][0]) == 3 and len(want[0]["seed_rows"]) == 1            # more present classes than rows


def test_roi_label_draws_its_own_permutation(cuda):
    """perm=None: torch.randperm on the device with the given generator — a permutation of every image's rows, and
    the labels are those of passing that permutation in."""
    case, _ = _label_reference([2000, 1500], "raw")
    g = torch.Generator(device=cuda).manual_seed(5)
    drawn = _device_label(case, "raw", cuda, perm=None, generator=g)
    perm = drawn["perm"]
    assert perm.is_cuda and perm.dtype == torch.int32 and perm.numel() == 3500
    assert torch.equal(torch.sort(perm[:2000]).values.cpu(), torch.arange(2000, dtype=torch.int32))
    assert torch.equal(torch.sort(perm[2000:]).values.cpu(), torch.arange(1500, dtype=torch.int32))
    assert not torch.equal(perm[:2000].cpu(), torch.arange(2000, dtype=torch.int32))
    again = _device_label(case, "raw", cuda, perm=perm)
    assert torch.equal(again["labels"], drawn["labels"]) and torch.equal(again["weights"], drawn["weights"])
    g2 = torch.Generator(device=cuda).manual_seed(5)
    assert torch.equal(_device_label(case, "raw", cuda, perm=None, generator=g2)["perm"], perm)
    other = _device_label(case, "raw", cuda)                                          # the case's own order: other picks
    assert not torch.equal(other["weights"], drawn["weights"])


def test_roi_label_refuses_fg_below_bg_hi(cuda):
    from jtsm_amd.layers.cmil import roi_label

    case, _ = _label_reference([39], "raw")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    with pytest.raises(ValueError):
        roi_label(t(case["S"]), t(case["boxes"]), t(case["offsets"]), t(case["classes"]), t(case["counts"]), t(case["CW"]),
                  perm=t(case["perm"]), fg=0.3, bg_hi=0.4)


# ---- against the reference's own compiled host operators (tests/golden/cmil_reference_cases.npz) ----------------------
def test_device_reproduces_the_recorded_reference_cases(cuda):
    import os

    from conftest import GOLDEN
    from jtsm_amd.layers.cmil import getlambda, roi_label, roi_merge

    z = np.load(os.path.join(GOLDEN, "cmil_reference_cases.npz"))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    for k in range(8):
        g = lambda name: z["merge%d_%s" % (k, name)]  # noqa: E731
        cur_iter, max_epoch, size_epoch = g("iters").tolist()
        n, live = g("S").shape[0], g("MC").shape[0]
        C, D = t(g("C")).requires_grad_(True), t(g("D")).requires_grad_(True)
        off = torch.tensor([0, n], dtype=torch.int32, device=cuda)
        MC, MD, I, IC, moff = roi_merge(t(g("S")), t(g("boxes")), C, D, off, getlambda(cur_iter, size_epoch, max_epoch), n)
        assert moff.cpu().tolist() == [0, live], k
        assert np.array_equal(I.cpu().numpy(), g("I")) and np.array_equal(IC.cpu().numpy(), g("IC")), k
        assert np.array_equal(MC.detach().cpu().numpy()[:live], g("MC")), k
        assert np.array_equal(MD.detach().cpu().numpy()[:live], g("MD")), k
        up = np.zeros((2, n) + g("MC").shape[1:], np.float32)
        up[:, :live] = g("gM")
        ((MC * t(up[0])).sum() + (MD * t(up[1])).sum()).backward()
        assert np.array_equal(C.grad.cpu().numpy(), g("GC")) and np.array_equal(D.grad.cpu().numpy(), g("GD")), k
    for k in range(6):
        g = lambda name: z["label%d_%s" % (k, name)]  # noqa: E731
        n = g("S").shape[0]
        ids = np.nonzero(g("L")[0] == 1)[0].astype(np.int32)
        classes = np.zeros((1, 20), np.int32)
        classes[0, :len(ids)] = ids
        out = roi_label(t(g("S")), t(g("boxes")), torch.tensor([0, n], dtype=torch.int32, device=cuda), t(classes),
                        torch.tensor([len(ids)], dtype=torch.int32, device=cuda), t(g("CW")[None]), rows_per_image=[n],
                        generator=torch.Generator(device=cuda).manual_seed(k), num_classes=20)
        assert np.array_equal(out["labels"].cpu().numpy(), g("RL")), k
        assert np.array_equal(out["weights"].cpu().numpy(), g("RW")), k
