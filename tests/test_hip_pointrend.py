"""GPU suite: the PointRend kernels (jtsm_amd/csrc/point_rend.hip) against the host restatement
(tests/pointrend_ref.py) and the vectors recorded from the reference (tests/golden/pointrend_reference_cases.npz).
Float quantities within the recorded bars; chosen points and cells as sets on every roi that is not ambiguous within
the recorded margin (at most 5 % of a case's rois), their order the restatement's; accuracy counts identical."""
import numpy as np
import pytest
import torch

import pointrend_ref as PR

pytestmark = pytest.mark.gpu

from jtsm_amd.layers import point_rend as P  # noqa: E402

CL = torch.channels_last
Z, META = PR.golden()


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def maps(fine, cuda, grad=False):
    return [dev(f, cuda).contiguous(memory_format=CL).requires_grad_(grad) for f in fine]


def sources(fine_t, scales, coarse_t):
    out, col = [], 0
    for f, s in zip(fine_t, scales):
        out.append((f, P.SHARED, s, col))
        col += f.shape[1]
    if coarse_t is not None:
        out.append((coarse_t, P.PER_ROI, 1.0, col))
    return out


def sets_equal(mine, recorded, amb):
    assert amb.mean() <= META["ambiguous_cap"]
    for r in range(len(mine)):
        if not amb[r]:
            assert np.array_equal(np.sort(mine[r]), recorded[r]), r


# ---- gather -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PR.GATHER_CASES))
def test_gather_recorded(cuda, name):
    fine, scales, coarse, boxes, roi_image, points = PR.gather_inputs(name, int(Z["gather_%s_seed" % name]))
    src = sources(maps(fine, cuda), scales, None if coarse is None else dev(coarse, cuda))
    rows, coords = P.point_gather(src, dev(boxes, cuda), dev(roi_image, cuda), dev(points, cuda))
    want, want_c = PR.gather(fine, scales, coarse, boxes, roi_image, points)
    assert np.abs(rows.cpu().numpy() - want).max() <= META["gather_bar"]
    assert np.abs(rows.cpu().numpy() - Z["gather_%s_rows" % name]).max() <= META["gather_bar"]
    assert np.abs(coords.cpu().numpy() - want_c).max() <= META["coords_bar"]
    assert np.abs(coords.cpu().numpy() - Z["gather_%s_coords" % name]).max() <= META["coords_bar"]


def test_gather_reference_names(cuda):
    """The functions with the reference's names return its shapes: (R, C, P) views of the points-major rows."""
    fine, scales, coarse, boxes, roi_image, points = PR.gather_inputs("one", 11)
    counts = np.bincount(roi_image, minlength=2)
    split = [dev(b, cuda) for b in np.split(boxes, np.cumsum(counts)[:-1])]
    feats, coords = P.point_sample_fine_grained_features(maps(fine, cuda), scales, split, dev(points, cuda))
    cf = P.point_sample(dev(coarse, cuda), dev(points, cuda), align_corners=False)
    want, want_c = PR.gather(fine, scales, coarse, boxes, roi_image, points)
    R, Pn = points.shape[:2]
    assert tuple(feats.shape) == (R, 5, Pn) and tuple(cf.shape) == (R, 5, Pn) and tuple(coords.shape) == (R, Pn, 2)
    got = torch.cat([feats, cf], 1).permute(0, 2, 1).reshape(R * Pn, -1).cpu().numpy()
    assert np.abs(got - want).max() <= META["gather_bar"]
    assert np.abs(P.get_point_coords_wrt_image(dev(boxes, cuda), dev(points, cuda)).cpu().numpy() - want_c).max() \
        <= META["coords_bar"]
    grid = dev(points[:, :6].reshape(R, 2, 3, 2), cuda)
    assert tuple(P.point_sample(dev(coarse, cuda), grid).shape) == (R, 5, 2, 3)
    with pytest.raises(NotImplementedError):
        P.point_sample(dev(coarse, cuda), dev(points, cuda), align_corners=True)


def test_gather_no_rois(cuda):
    fine = [np.random.RandomState(0).randn(2, 5, 13, 9).astype(np.float32)]
    f = maps(fine, cuda, grad=True)
    feats, coords = P.point_sample_fine_grained_features(f, [0.25], [torch.zeros((0, 4), device=cuda)] * 2,
                                                         torch.zeros((0, 7, 2), device=cuda))
    assert tuple(feats.shape) == (0, 5, 7) and tuple(coords.shape) == (0, 7, 2)
    feats.sum().backward()
    assert float(f[0].grad.abs().sum()) == 0.0


def test_gather_columns_and_untouched_rest(cuda):
    """The fine and the coarse part land at their column offsets of a wider row buffer; the other columns keep what
    they held."""
    fine, scales, coarse, boxes, roi_image, points = PR.gather_inputs("one", 12)
    R, Pn = points.shape[:2]
    out = torch.full((R * Pn, 24), -7.0, device=cuda)
    src = [(maps(fine, cuda)[0], P.SHARED, scales[0], 3), (dev(coarse, cuda), P.PER_ROI, 1.0, 16)]
    rows, _ = P.point_gather(src, dev(boxes, cuda), dev(roi_image, cuda), dev(points, cuda), out=out)
    assert rows.data_ptr() == out.data_ptr()
    want, _ = PR.gather(fine, scales, coarse, boxes, roi_image, points)
    got = out.cpu().numpy()
    assert np.abs(got[:, 3:8] - want[:, :5]).max() <= META["gather_bar"]
    assert np.abs(got[:, 16:21] - want[:, 5:]).max() <= META["gather_bar"]
    rest = np.r_[0:3, 8:16, 21:24]
    assert np.all(got[:, rest] == -7.0)


@pytest.mark.parametrize("s2d", [False, True])
def test_gather_grid_mode(cuda, s2d):
    """The 14 x 14 grid mode equals the plain mode on generate_regular_grid_point_coords, up to the space-to-depth
    permutation of the rows."""
    fine, scales, coarse, boxes, roi_image, _ = PR.gather_inputs("two", 13)
    R = len(boxes)
    f = maps(fine, cuda)
    src = sources(f, scales, None)
    pts = P.generate_regular_grid_point_coords(R, 14, cuda).contiguous()
    assert np.abs(pts[0].cpu().numpy() - PR.grid_points(14)).max() <= 1e-6
    plain, pc = P.point_gather(src, dev(boxes, cuda), dev(roi_image, cuda), pts)
    grid, gc = P.point_gather(src, dev(boxes, cuda), dev(roi_image, cuda), grid_side=14, space_to_depth=s2d)
    q = np.arange(196)
    blk = q >> 2
    perm = (2 * (blk // 7) + ((q >> 1) & 1)) * 14 + 2 * (blk % 7) + (q & 1) if s2d else q
    perm = torch.from_numpy(perm).to(cuda)
    assert torch.equal(grid.view(R, 196, -1), plain.view(R, 196, -1)[:, perm])
    assert torch.equal(gc, pc[:, perm])


@pytest.mark.parametrize("name", ["one", "two"])
def test_gather_backward(cuda, name):
    fine, scales, coarse, boxes, roi_image, points = PR.gather_inputs(name, int(Z["gather_%s_seed" % name]))
    f = maps(fine, cuda, grad=True)
    c = dev(coarse, cuda).requires_grad_(True)
    rows, _ = P.point_gather(sources(f, scales, c), dev(boxes, cuda), dev(roi_image, cuda), dev(points, cuda))
    g = np.random.RandomState(1).randn(*rows.shape).astype(np.float32)
    rows.backward(dev(g, cuda))
    wf, wc = PR.gather_adjoint(g.astype(np.float64), [x.shape for x in fine], scales, coarse.shape, boxes, roi_image,
                               points)
    for got, want in list(zip([x.grad for x in f], wf)) + [(c.grad, wc)]:
        assert np.abs(got.cpu().numpy() - want).max() <= META["grad_bar"] * np.abs(want).max()


def test_gather_backward_grid_mode(cuda):
    fine, scales, _, boxes, roi_image, _ = PR.gather_inputs("one", 14)
    f = maps(fine, cuda, grad=True)
    R = len(boxes)
    rows, _ = P.point_gather(sources(f, scales, None), dev(boxes, cuda), dev(roi_image, cuda), grid_side=14,
                             space_to_depth=True)
    g = np.random.RandomState(2).randn(*rows.shape).astype(np.float32)
    rows.backward(dev(g, cuda))
    pts = np.tile(PR.grid_points(14, True)[None], (R, 1, 1))
    wf, _ = PR.gather_adjoint(g.astype(np.float64), [fine[0].shape], scales, None, boxes, roi_image, pts)
    assert np.abs(f[0].grad.cpu().numpy() - wf[0]).max() <= META["grad_bar"] * np.abs(wf[0]).max()


def test_gather_backward_is_deterministic_on_a_pile(cuda):
    """All points of all rois in one cell: the gradient is the same bits twice, for the shared map and the coarse one."""
    rng = np.random.RandomState(3)
    fine = [rng.randn(1, 40, 13, 9).astype(np.float32)]
    coarse = rng.randn(6, 5, 7, 7).astype(np.float32)
    boxes = np.tile(np.array([[9, 9, 13, 13]], np.float32), (6, 1))
    points = (0.5 + 0.01 * rng.uniform(-1, 1, (6, 196, 2))).astype(np.float32)
    g = dev(rng.randn(6 * 196, 45).astype(np.float32), cuda)
    got = []
    for _ in range(2):
        f, c = maps(fine, cuda, grad=True), dev(coarse, cuda).requires_grad_(True)
        rows, _ = P.point_gather(sources(f, [0.25], c), dev(boxes, cuda), torch.zeros(6, dtype=torch.int32, device=cuda),
                                 dev(points, cuda))
        rows.backward(g)
        got.append((f[0].grad.clone(), c.grad.clone()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert int((got[0][0] != 0).any(1).sum()) <= 4          # one pile: a 2 x 2 block of cells


def test_gather_backward_through_the_fan(cuda):
    """A shared map with a second reader: the gather adds its term into the fan's map."""
    from jtsm_amd.layers import grad_fan
    fine, scales, _, boxes, roi_image, points = PR.gather_inputs("one", 15)
    x = maps(fine, cuda, grad=True)[0]
    a, b = grad_fan.fan_out(x, 2)
    r1, _ = P.point_gather([(a, P.SHARED, scales[0], 0)], dev(boxes, cuda), dev(roi_image, cuda), dev(points, cuda))
    r2, _ = P.point_gather([(b, P.SHARED, scales[0], 0)], dev(boxes, cuda), dev(roi_image, cuda), dev(points, cuda))
    g = np.random.RandomState(4).randn(*r1.shape).astype(np.float32)
    ((r1 + 2 * r2) * dev(g, cuda)).sum().backward()
    wf, _ = PR.gather_adjoint(3 * g.astype(np.float64), [fine[0].shape], scales, None, boxes, roi_image, points)
    assert np.abs(x.grad.cpu().numpy() - wf[0]).max() <= META["grad_bar"] * np.abs(wf[0]).max()


# ---- selection --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PR.SELECT_CASES))
def test_select_recorded(cuda, name):
    coarse, classes, cand, rand, Pn, U = PR.select_inputs(name, int(Z["select_%s_seed" % name]))
    pts, chosen = P.point_select(dev(coarse, cuda), dev(classes, cuda), dev(cand, cuda),
                                 None if rand is None else dev(rand, cuda), Pn, return_chosen=True)
    pts, chosen = pts.cpu().numpy(), chosen.cpu().numpy()
    _, _, u = PR.select(coarse, classes, cand, rand, U)
    amb = PR.ambiguous(u, U, META["select_margin"])
    sets_equal(chosen, Z["select_%s_chosen" % name], amb)
    # the order is the restatement's on the float32 values the kernel ranks: uncertainty descending, index ascending
    assert np.array_equal(chosen, PR.select(coarse, classes, cand, rand, U, PR.F32)[1])
    for r in range(len(u)):
        assert np.array_equal(pts[r, :U], cand[r, chosen[r]])
    if rand is not None:
        assert np.array_equal(pts[:, U:], rand)
        assert np.array_equal(pts[:, U:], Z["select_%s_coords" % name][:, U:])


def test_select_order_is_the_float32_restatement(cuda):
    coarse, classes, cand, rand, Pn, U = PR.select_inputs("shipped", 7)
    _, chosen = P.point_select(dev(coarse, cuda), dev(classes, cuda), dev(cand, cuda), dev(rand, cuda), Pn,
                               return_chosen=True)
    _, want, _ = PR.select(coarse, classes, cand, rand, U, PR.F32)
    assert np.array_equal(chosen.cpu().numpy(), want)


@pytest.mark.parametrize("C", [1, 5])
def test_select_constant_map_ties(cuda, C):
    """Every uncertainty ties (a map of zeros samples exactly 0 everywhere): the lower candidate index goes first."""
    coarse, classes, cand, rand, Pn, U = PR.select_inputs("p8c5", 8)
    coarse = np.zeros((3, C, 7, 7), np.float32)
    pts, chosen = P.point_select(dev(coarse, cuda), dev(classes, cuda), dev(cand, cuda), dev(rand, cuda), Pn,
                                 return_chosen=True)
    _, want, _ = PR.select(coarse, classes % C, cand, rand, U, PR.F32)
    assert np.array_equal(want, np.tile(np.arange(U), (3, 1)))
    assert np.array_equal(chosen.cpu().numpy(), want)
    assert np.array_equal(pts.cpu().numpy()[:, :U], cand[:, :U])


def test_select_seeded_wrapper_draws_the_reference_numbers(cuda):
    """get_uncertain_point_coords_with_randomness calls torch.rand twice, with the reference's shapes in its order."""
    coarse, classes, _, _, Pn, U = PR.select_inputs("p8c5", 9)
    torch.manual_seed(5)
    got = P.get_uncertain_point_coords_with_randomness(dev(coarse, cuda), P.UncertaintyOfClasses(dev(classes, cuda)),
                                                       Pn, 3, 0.75)
    torch.manual_seed(5)
    cand = torch.rand(3, 24, 2, device=cuda)
    rand = torch.rand(3, Pn - U, 2, device=cuda)
    want = P.point_select(dev(coarse, cuda), dev(classes, cuda), cand, rand, Pn)
    assert torch.equal(got, want) and torch.equal(got[:, U:], rand)
    with pytest.raises(NotImplementedError):
        P.get_uncertain_point_coords_with_randomness(dev(coarse, cuda), lambda x: -x.abs(), Pn, 3, 0.75)


# ---- loss -------------------------------------------------------------------------------------------------------------
def run_loss(cuda, args):
    logits, classes, masks, roi_image, matched, coords, Pn = args
    x = dev(logits, cuda).requires_grad_(True)
    loss, stats, targets = P.point_loss(x, dev(classes, cuda), [None if m is None else dev(m, cuda) for m in masks],
                                        dev(roi_image, cuda), dev(matched, cuda), dev(coords, cuda), Pn,
                                        return_details=True)
    loss.backward()
    return float(loss.detach()), x.grad.cpu().numpy(), targets.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize("name", list(PR.LOSS_CASES))
def test_loss_recorded(cuda, name):
    args = PR.loss_inputs(name, int(Z["loss_%s_seed" % name]))
    loss, grad, targets, stats = run_loss(cuda, args)
    wl, wg, wt, wa = PR.point_loss(*args)
    assert abs(loss - wl) <= META["loss_bar"] and abs(loss - float(Z["loss_%s_loss" % name])) <= META["loss_bar"]
    assert np.abs(grad - wg).max() <= META["loss_grad_bar"] * np.abs(wg).max()
    assert np.abs(grad - Z["loss_%s_grad" % name]).max() <= META["loss_grad_bar"] * np.abs(wg).max()
    assert np.abs(targets - wt).max() <= META["target_bar"]
    assert stats[0] == wa == int(Z["loss_%s_accurate" % name]) and stats[1] == len(wt)
    C = args[0].shape[1]
    col = np.repeat(args[1] if C > 1 else np.zeros_like(args[1]), args[6])
    off = np.ones_like(grad, bool)
    off[np.arange(len(col)), col] = False
    assert np.all(grad[off] == 0)


def test_loss_accuracy_at_a_target_of_one(cuda):
    """Inside an all-ones mask the four weights sum to exactly 1.0 or to just below it, and uint8() of the latter is 0:
    the count follows the float32 sum as the kernel forms it."""
    rng = np.random.RandomState(5)
    Pn = 2000
    masks = [np.ones((1, 37, 53), np.uint8)]
    coords = np.stack([rng.uniform(2, 51, Pn), rng.uniform(2, 35, Pn)], -1).astype(np.float32)[None]
    t32 = PR.soft_targets(masks, [0], [0], coords, PR.F32).reshape(-1)
    assert (t32 == 1).sum() > 10 and ((t32 < 1) & (t32 > 1 - 1e-6)).sum() > 10
    logits = np.ones((Pn, 1), np.float32)
    args = (logits, np.zeros(1, np.int64), masks, np.zeros(1, np.int32), np.zeros(1, np.int32), coords, Pn)
    _, _, targets, stats = run_loss(cuda, args)
    assert np.array_equal(targets, t32)
    assert stats[0] == int((t32 >= 1).sum()) == PR.point_loss(*args)[3]


def test_loss_without_rois(cuda):
    x = torch.zeros((0, 5), device=cuda, requires_grad=True)
    e = torch.zeros(0, dtype=torch.int32, device=cuda)
    loss, stats, _ = P.point_loss(x, e.long(), [None, None], e, e, torch.zeros((0, 7, 2), device=cuda), 7,
                                  return_details=True)
    loss.backward()
    assert float(loss.detach()) == 0.0 and tuple(x.grad.shape) == (0, 5) and stats.cpu().tolist() == [0, 0]


def test_loss_reference_signature(cuda):
    """roi_mask_point_loss(mask_logits (R, C, P), instances, points_coord) on the rois' own bitmasks."""
    from jtsm_amd.structures import Instances
    args = PR.loss_inputs("two", 21)
    logits, classes, masks, roi_image, matched, coords, Pn = args
    R, C = len(roi_image), logits.shape[1]
    inst = []
    for n, m in enumerate(masks):
        rows = np.nonzero(roi_image == n)[0]
        i = Instances((m.shape[1], m.shape[2]))
        i.gt_masks = dev(m[matched[rows]], cuda)
        i.gt_classes = dev(classes[rows], cuda)
        inst.append(i)
    x = dev(logits, cuda).view(R, Pn, C).permute(0, 2, 1)
    loss = P.roi_mask_point_loss(x, inst, dev(coords, cuda))
    assert abs(float(loss) - PR.point_loss(*args)[0]) <= META["loss_bar"]
    none = Instances((4, 4))
    none.gt_classes = torch.zeros(0, dtype=torch.int64, device=cuda)
    assert float(P.roi_mask_point_loss(x[:0], [none], dev(coords[:0], cuda))) == 0.0


# ---- subdivision ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PR.SUBDIV_CASES))
def test_subdivide_recorded(cuda, name):
    m, N = PR.subdiv_inputs(name, int(Z["subdiv_%s_seed" % name]))
    n = PR.step_points(m.shape[1], m.shape[2], N)
    up, idx, coords = P.point_subdivide(dev(m, cuda)[:, None], n)
    wu, wi, wc = PR.subdivide(m, n)
    up = up[:, 0].cpu().numpy()
    assert np.abs(up - wu).max() <= META["up_bar"]
    s = int(Z["subdiv_%s_stride" % name])
    assert np.abs(up[:, ::s, ::s] - Z["subdiv_%s_up" % name]).max() <= META["up_bar"]
    if n == 0:
        assert idx is None and coords is None
        return
    idx, coords = idx.cpu().numpy(), coords.cpu().numpy()
    amb = PR.ambiguous(-np.abs(wu).reshape(len(m), -1), wi.shape[1], META["subdiv_margin"])
    sets_equal(idx, Z["subdiv_%s_chosen" % name], amb)
    # the order: the restatement's on the kernel's own float32 map
    mine, mine_c = PR.grid_topk(-np.abs(up), n)
    assert np.array_equal(idx, mine) and np.array_equal(coords, mine_c)
    if wi.shape[1] == up.shape[1] * up.shape[2]:
        assert all(np.array_equal(np.sort(row), np.arange(wi.shape[1])) for row in idx)      # all cells chosen


def test_subdivide_constant_map_ties(cuda):
    m = np.full((3, 14, 14), 1.5, np.float32)
    _, idx, coords = P.point_subdivide(dev(m, cuda)[:, None], 100)
    assert np.array_equal(idx.cpu().numpy(), np.tile(np.arange(100), (3, 1)))
    assert np.array_equal(coords.cpu().numpy(), PR.grid_topk(np.zeros((3, 28, 28)), 100)[1])


def test_topk_on_a_given_grid(cuda):
    u = np.random.RandomState(6).randn(3, 13, 9).astype(np.float32)
    u[1] = np.round(u[1])                       # ties
    idx, coords = P.get_uncertain_point_coords_on_grid(dev(u, cuda)[:, None], 20)
    wi, wc = PR.grid_topk(u, 20)
    assert np.array_equal(idx.cpu().numpy(), wi) and np.array_equal(coords.cpu().numpy(), wc)


def test_scatter(cuda):
    rng = np.random.RandomState(7)
    m = rng.randn(3, 1, 8, 8).astype(np.float32)
    idx = np.stack([rng.permutation(64)[:10] for _ in range(3)])
    rows = rng.randn(30, 5).astype(np.float32)
    cls = np.array([4, 0, 2])
    got = P.point_scatter(dev(m, cuda), dev(idx, cuda), dev(rows, cuda), dev(cls, cuda)).cpu().numpy()
    want = m.copy().reshape(3, 64)
    for r in range(3):
        want[r, idx[r]] = rows[r * 10:(r + 1) * 10, cls[r]]
    assert np.array_equal(got.reshape(3, 64), want)


def run_loop(cuda, coarse, classes, fine, scales, boxes, roi_image, weight, steps, N):
    """The five-step loop on the device, one channel, with a fixed small point head (one 1x1 layer as a matmul)."""
    R, C = coarse.shape[:2]
    ct, cls = dev(coarse, cuda), dev(classes, cuda)
    f = maps(fine, cuda)
    m = ct[torch.arange(R, device=cuda), cls][:, None].contiguous()
    w = dev(weight.astype(np.float32), cuda)
    for step in range(steps):
        H, W = m.shape[-2:]
        n = PR.step_points(H, W, N, step == steps - 1)
        m, idx, coords = P.point_subdivide(m, n)
        if n == 0:
            continue
        rows, _ = P.point_gather(sources(f, scales, ct), dev(boxes, cuda), dev(roi_image, cuda), coords,
                                 want_coords=False)
        P.point_scatter(m, idx, rows @ w, cls)
    return m[:, 0].cpu().numpy()


def test_whole_loop_equals_the_predicted_channel_of_all_channels(cuda):
    """R = 3, C = 5, a 32 x 32 feature map, five steps: the one-channel result on the device equals the predicted
    class's channel of the all-channel restatement on every roi that is unambiguous at every step."""
    rng = np.random.RandomState(9)
    R, C, N, steps = 3, 5, 784, 5
    fine = [rng.randn(1, 8, 32, 32).astype(np.float32)]
    coarse = (4 * rng.randn(R, C, 7, 7)).astype(np.float32)
    classes = rng.randint(0, C, R)
    boxes = np.array([[10, 12, 90, 100], [-6, 30, 60, 140], [40, 40, 120, 70]], np.float32)
    roi_image = np.zeros(R, np.int32)
    weight = rng.randn(8 + C, C)

    def point_fn(coords):
        pts = coords.astype(np.float32)
        rows, _ = PR.gather(fine, [0.25], coarse, boxes, roi_image, pts)
        return (rows @ weight).reshape(R, -1, C)

    full, amb = PR.subdivision_loop(coarse, classes, point_fn, steps, N, False, META["subdiv_margin"])
    got = run_loop(cuda, coarse, classes, fine, [0.25], boxes, roi_image, weight, steps, N)
    assert got.shape == (R, 224, 224)
    keep = ~amb
    assert keep.sum() >= 2
    # a cell holds an up-sampled value (up_bar) or a point logit: 13 gathered features, each within gather_bar, times
    # the fixed head's weights, summed in float32 (13 roundings of 2^-24 relative to the largest partial sum)
    logit_bar = META["gather_bar"] * np.abs(weight).sum(0).max() + 13 * 2.0 ** -24 * np.abs(full).max() * 13
    assert np.abs(got[keep] - full[keep]).max() <= max(META["up_bar"], logit_bar)


def test_zero_detections(cuda):
    m = torch.zeros((0, 1, 7, 7), device=cuda)
    up, idx, coords = P.point_subdivide(m, 10)
    assert tuple(up.shape) == (0, 1, 14, 14) and tuple(idx.shape) == (0, 10) and tuple(coords.shape) == (0, 10, 2)
