"""GPU suite (pytest -m gpu): mine_top_p (jtsm_amd/csrc/mist.hip) + match_label against the torch-CPU restatement
of get_pgt_top_k(0.15) + get_pgt_mist + label_and_sample_proposals (tests/mist_ref.py), and the OICR loss with
SMOOTH_L1_BETA against its torch expression.

Cases are (rows per image, present classes per image), proposals piled around a few rectangles, in three modes: raw
scores (branch 0), logits + lse + deltas (a later branch with regression), logits + lse alone (without: the reference
decodes zero deltas).  The kernels have no single-workgroup capacity — no per-list state lives in LDS — so the cases
cover the sizes at which they loop instead: more than 1024 candidates (a second NMS chunk, a second ranking workgroup),
more than 4096 rows (a second LDS tile of keys), more than 8192 rows (a second pass of owned rows), and candidate
counts of 64 n +- 1 (the last wavefront's ballot).

rows, classes, num and the labels / matched indices of the following match_label are compared bit for bit, and so are
scores and boxes in the raw mode; in the logits modes probabilities and decoded boxes take the tolerance
tests/test_hip_losses.py applies to mine_top1's (scores rtol 1e-4 atol 1e-7, boxes rtol 1e-5 atol 1e-3).  Every case
meets mist_ref.well_defined, asserted by the generator, which may discard at most half of the seeds it tries."""
import pytest
import torch

import mist_ref as MR

pytestmark = pytest.mark.gpu

CASES = [([7], [1]), ([20, 333], [2, 1]), ([333, 100], [3, 0]), ([2000, 1500], [1, 6]), ([4500], [5]),
         ([434, 425], [1, 1]), ([8300], [2])]
MODES = ["raw", "reg", "noreg"]
K = 20


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch.device("cuda", 0)


_REF = {}


def _reference(rows, classes, mode):
    """(case, per-image restatement results), computed once per (case, mode) and shared."""
    key = (tuple(rows), tuple(classes), mode)
    if key not in _REF:
        case, tried = MR.generate(rows, classes, mode, K=K)
        assert tried <= 2, "the generator discarded %d of %d seeds" % (tried - 1, tried)
        want = []
        for i in range(len(rows)):
            m = MR.mist(*MR.image_inputs(case, i), case["class_ids"][i])
            want.append((m, MR.label(case["boxes"][i], m, K)))
        _REF[key] = (case, want)
    return _REF[key]


def _device_run(case, cuda):
    from jtsm_amd.layers.mining import match_label, pad_class_lists, row_lse
    from jtsm_amd.layers.mist import mine_top_p, top_p_counts

    rows = case["rows"]
    boxes = torch.cat(case["boxes"]).to(cuda)
    off = torch.tensor([0] + list(torch.tensor(rows).cumsum(0)), dtype=torch.int32, device=cuda)
    cls, cnt, _ = pad_class_lists([c.to(cuda) for c in case["class_ids"]], cuda)
    top_t, t_max = top_p_counts(rows, 0.15, cuda)
    sc = case["scores"].to(cuda)
    if case["mode"] == "raw":
        pg = mine_top_p(sc, boxes, off, cls, cnt, top_t, t_max)
    else:
        dl = case["deltas"].to(cuda) if case["deltas"] is not None else None
        pg = mine_top_p(sc, boxes, off, cls, cnt, top_t, t_max, lse=row_lse(sc), deltas=dl)
    lab = match_label(boxes, off, pg, pg["classes"], pg["num"], K)
    return pg, lab


def _compare(case, want, pg, lab):
    pg = {k: v.cpu() for k, v in pg.items()}
    lab = {k: v.cpu() for k, v in lab.items()}
    lo = 0
    for i, (m, l) in enumerate(want):
        n, k = case["rows"][i], len(m["rows"])
        assert int(pg["num"][i]) == k, (i, int(pg["num"][i]), k)
        assert torch.equal(pg["rows"][i, :k].long(), m["rows"]), i
        assert torch.equal(pg["classes"][i, :k].long(), m["classes"]), i
        if case["mode"] == "raw":
            assert torch.equal(pg["scores"][i, :k], m["scores"]) and torch.equal(pg["boxes"][i, :k], m["boxes"]), i
        else:
            assert torch.allclose(pg["scores"][i, :k], m["scores"], rtol=1e-4, atol=1e-7), i
            assert torch.allclose(pg["boxes"][i, :k], m["boxes"], rtol=1e-5, atol=1e-3), i
        assert torch.equal(pg["weights"][i], pg["scores"][i])                     # gt_weights = pgt_scores
        for name in ("rows", "classes", "scores", "weights", "boxes"):            # zero-filled padding
            assert not pg[name][i, k:].any(), (i, name)
        assert torch.equal(lab["labels"][lo:lo + n].long(), l["classes"]), i
        assert torch.equal(lab["matched"][lo:lo + n].long(), l["idx"]), i
        if k == 0:
            assert (lab["weights"][lo:lo + n] == 0).all()
        lo += n


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows,classes", CASES, ids=["-".join(map(str, r)) for r, _ in CASES])
def test_mining_and_labelling_match_the_restatement(cuda, rows, classes, mode):
    case, want = _reference(rows, classes, mode)
    pg, lab = _device_run(case, cuda)
    t_max = max(MR.top_t(n, 0.15) for n in rows)
    assert pg["boxes"].shape == (len(rows), t_max * max(max(classes), 1), 4)
    _compare(case, want, pg, lab)


def test_zero_delta_decode_differs_from_the_proposal_row_and_is_what_is_emitted(cuda):
    """A branch without regression: the box is apply_deltas(0, proposal), not the proposal — the two differ in the
    last bit on some rows, and the emitted boxes are the decoded ones, bit for bit where decode_box and the torch
    expression agree (they share the operation order; exp(0) = 1)."""
    from oracle import model as OM

    case, want = _reference([333, 100], [3, 0], "noreg")
    pg, _ = _device_run(case, cuda)
    b = case["boxes"][0]
    dec = OM.apply_deltas(torch.zeros(len(b), 4), b)
    assert not torch.equal(dec, b)
    k = int(pg["num"][0])
    assert torch.equal(pg["boxes"][0, :k].cpu(), dec[pg["rows"][0, :k].cpu().long()])


def test_ties_go_to_the_lower_row_and_the_lower_list_index(cuda):
    """Equal scores and duplicate boxes: among equal class scores the lower row is the earlier candidate, among equal
    candidate scores the lower list index is visited first (and suppresses its duplicates) — the restatement sorts
    stably.  A grid of disjoint cells keeps hundreds of survivors, spread over several NMS chunks."""
    from jtsm_amd.layers.mining import pad_class_lists
    from jtsm_amd.layers.mist import mine_top_p, top_p_counts

    g = torch.Generator().manual_seed(5)
    n, ids = 4000, torch.tensor([2, 9, 11])
    cell = torch.randint(0, 900, (n,), generator=g)              # many rows share a cell: duplicate boxes
    x, y = (cell % 30).float() * 40.0, (cell // 30).float() * 40.0
    boxes = torch.stack([x, y, x + 30.0, y + 30.0], 1)
    scores = torch.randint(1, 40, (n, K), generator=g).float() / 64.0        # 39 levels: ties everywhere
    scores[:, 9] = scores[:, 2]                                  # two classes with the same column: cross-class ties
    m = MR.mist(boxes[:, None, :].expand(n, K, 4), scores, ids)
    assert len(m["rows"]) > 300
    off = torch.tensor([0, n], dtype=torch.int32, device=cuda)
    cls, cnt, _ = pad_class_lists([ids.to(cuda)], cuda)
    top_t, t_max = top_p_counts([n], 0.15, cuda)
    pg = {k: v.cpu() for k, v in mine_top_p(scores.to(cuda), boxes.to(cuda), off, cls, cnt, top_t, t_max).items()}
    k = len(m["rows"])
    assert int(pg["num"][0]) == k
    assert torch.equal(pg["rows"][0, :k].long(), m["rows"]) and torch.equal(pg["classes"][0, :k].long(), m["classes"])
    assert torch.equal(pg["scores"][0, :k], m["scores"]) and torch.equal(pg["boxes"][0, :k], m["boxes"])


def test_two_runs_agree_in_every_bit(cuda):
    case, _ = _reference([2000, 1500], [1, 6], "reg")
    a, la = _device_run(case, cuda)
    b, lb = _device_run(case, cuda)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    for k in la:
        assert torch.equal(la[k].view(torch.int32), lb[k].view(torch.int32)), k


def test_mining_and_labelling_never_synchronise(cuda):
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch has no torch.cuda.set_sync_debug_mode")
    from jtsm_amd.layers.mining import match_label, pad_class_lists, row_lse
    from jtsm_amd.layers.mist import mine_top_p, top_p_counts

    case, want = _reference([20, 333], [2, 1], "reg")
    rows = case["rows"]
    boxes = torch.cat(case["boxes"]).to(cuda)
    off = torch.tensor([0] + list(torch.tensor(rows).cumsum(0)), dtype=torch.int32, device=cuda)
    cls, cnt, _ = pad_class_lists([c.to(cuda) for c in case["class_ids"]], cuda)
    sc, dl = case["scores"].to(cuda), case["deltas"].to(cuda)
    top_t, t_max = top_p_counts(rows, 0.15, cuda)
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:                                        # pragma: no cover
        pytest.skip("torch.cuda.set_sync_debug_mode is not supported on this backend: %s" % e)
    try:
        pg = mine_top_p(sc, boxes, off, cls, cnt, top_t, t_max, lse=row_lse(sc), deltas=dl)
        lab = match_label(boxes, off, pg, pg["classes"], pg["num"], K)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _compare(case, want, pg, lab)


# ---- OICR loss with SMOOTH_L1_BETA ------------------------------------------------------------------------------
def rel_close(a, b, tol=1e-4, what=""):
    """(the bar of tests/test_hip_losses.py's OICR loss test)"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    ref = b.abs().max().item() + 1e-30
    err = (a - b).abs().max().item()
    print("%s: err %.3e ref %.3e" % (what, err, ref))
    assert err <= tol * ref, "%s: err %.3e ref %.3e" % (what, err, ref)


def _smooth_l1_case(R=300, ncls=21):
    g = torch.Generator().manual_seed(31)
    kc = ncls - 1
    z = torch.randn(R, ncls, generator=g) * 2
    d = torch.randn(R, 4 * kc, generator=g) * 0.5
    labels = torch.randint(0, ncls, (R,), generator=g)
    labels[torch.rand(R, generator=g) < 0.5] = kc
    labels[:3] = torch.tensor([-1, 0, kc - 1])
    w = torch.rand(R, generator=g)
    w[torch.rand(R, generator=g) < 0.2] = 0.0
    prop = torch.rand(R, 4, generator=g) * 200
    prop[:, 2:] += prop[:, :2] + 4
    gt = prop + torch.randn(R, 4, generator=g) * 3
    gt[:, 2:] = torch.max(gt[:, 2:], gt[:, :2] + 2)
    return z, d, labels, w, prop, gt


def _cpu_oicr(z, d, labels, w, prop, gt, beta):
    """oracle.model.oicr_losses with detectron2's smooth_l1_loss(beta) in place of its beta = 0 form."""
    from oracle import model as OM

    kc = z.shape[1] - 1
    w = w.clone()
    w[labels == -1] = 0.0
    valid = (w > 1e-12).to(w.dtype).sum()
    ce = torch.nn.functional.cross_entropy(z, labels, reduction="none", ignore_index=-1)
    fg = torch.nonzero((labels >= 0) & (labels < kc))[:, 0]
    cols = 4 * labels[fg][:, None] + torch.arange(4)
    n = (d[fg[:, None], cols] - OM.box_deltas(prop, gt)[fg]).abs()
    l = n if beta < 1e-5 else torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
    return (ce * w).sum() / valid, (l * w[fg, None]).sum() / labels.numel()


@pytest.mark.parametrize("beta", [0.0, 1.0, 0.11])
def test_oicr_loss_with_smooth_l1_beta(cuda, beta):
    from jtsm_amd.layers.wsl_losses import oicr_loss
    z, d, labels, w, prop, gt = _smooth_l1_case()
    z0, d0 = z.clone().requires_grad_(), d.clone().requires_grad_()
    lc0, lb0 = _cpu_oicr(z0, d0, labels, w, prop, gt, beta)
    (lc0 * 0.7 + lb0 * 1.3).backward()
    zd, dd = z.to(cuda).requires_grad_(), d.to(cuda).requires_grad_()
    lc, lb = oicr_loss(zd, dd, labels.to(cuda), w.to(cuda), prop.to(cuda), gt.to(cuda), beta=beta)
    (lc * 0.7 + lb * 1.3).backward()
    rel_close(lc, lc0, what="loss_cls")
    rel_close(lb, lb0, what="loss_box")
    rel_close(zd.grad, z0.grad, what="dz")
    rel_close(dd.grad, d0.grad, what="dd")
    if beta == 0.0:                 # the bits of the original entry points
        ze, de = z.to(cuda).requires_grad_(), d.to(cuda).requires_grad_()
        lce, lbe = oicr_loss(ze, de, labels.to(cuda), w.to(cuda), prop.to(cuda), gt.to(cuda))
        (lce * 0.7 + lbe * 1.3).backward()
        assert torch.equal(lc, lce) and torch.equal(lb, lbe)
        assert torch.equal(zd.grad, ze.grad) and torch.equal(dd.grad, de.grad)
    else:                           # and the smooth form is not the L1 one
        assert float(lb) != float(_cpu_oicr(z, d, labels, w, prop, gt, 0.0)[1])
