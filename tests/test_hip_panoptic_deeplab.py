"""GPU suite: the Panoptic-DeepLab kernels of csrc/panoptic_deeplab.hip (layers/panoptic_deeplab.py, solver.Adam) against
tests/panoptic_deeplab_ref.py, the stock-torch CPU restatement that tests/test_panoptic_deeplab_ref.py pins to the
reference's own outputs.  Integer results (centres, instance ids, panoptic map, segment table, boxes, areas, centre
pixels) must be identical; float results have a bar of four times the error the torch fp32 formulation itself makes
against fp64 on the same input (the margin covers another summation order, nothing else)."""
import copy
import os

import numpy as np
import pytest
import torch

import panoptic_deeplab_ref as R

pytestmark = pytest.mark.gpu

from jtsm_amd.layers import panoptic_deeplab as P  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "panoptic_deeplab.npz")
CL = torch.channels_last


# ---- centres -----------------------------------------------------------------------------------------------------------
def _check_centres(heat, kernel, top_k, cuda, threshold=0.1):
    want = R.find_instance_center(heat.clone(), threshold, kernel, top_k)
    got = P.find_instance_center(heat.to(cuda), threshold, kernel, top_k)
    assert got.dtype == torch.int64 and got.shape == want.shape, (got.shape, want.shape)
    assert torch.equal(got.cpu(), want)
    centers, count = P._find_centers(heat[0].to(cuda).contiguous(), threshold, kernel, top_k)
    assert int(count) == want.shape[0] <= top_k - 1
    assert torch.equal(centers[:want.shape[0]].cpu().long(), want) and bool((centers[want.shape[0]:] == -1).all())
    return want


# 304 x 432 = 131328 pixels are 513 tiles of 256: the chunked passes run 257 workgroups of two tiles each, the regime of
# every map above 131072 pixels (the smaller shapes run one tile per workgroup)
ABOVE_256_WORKGROUPS = (304, 432)


def _random_map_cases():
    """Every small shape with every kernel and top_k (under the ids they have always had), and the large one once."""
    small = [pytest.param(shape, kernel, top_k, id="%d-%d-shape%d" % (top_k, kernel, i))
             for top_k in (5, 20, 200) for kernel in (3, 7) for i, shape in enumerate([(64, 96), (37, 53)])]
    return small + [pytest.param(ABOVE_256_WORKGROUPS, 3, 200, id="200-3-above_256_workgroups")]


@pytest.mark.parametrize("shape,kernel,top_k", _random_map_cases())
def test_centres_random_map(cuda, shape, kernel, top_k):
    g = torch.Generator().manual_seed(shape[0] * 100 + kernel * 10 + top_k)
    heat = torch.rand(1, *shape, generator=g)
    want = _check_centres(heat, kernel, top_k, cuda)
    candidates = R.find_instance_center(heat.clone(), 0.1, kernel, shape[0] * shape[1]).shape[0]   # (cut at 0)
    # distinct values: the cut drops exactly the top_k-th; fewer candidates than top_k: all of them stay
    assert want.shape[0] == (top_k - 1 if candidates >= top_k else candidates)


@pytest.mark.parametrize("shape", [(64, 96), (37, 53)])
@pytest.mark.parametrize("kernel", [3, 7])
def test_centres_few_candidates(cuda, shape, kernel):
    h, w = shape
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    heat = torch.zeros(h, w)
    for k, (cy, cx) in enumerate([(5, 7), (h // 2, w // 2), (h - 9, w - 20), (h // 3, w - 6)]):
        heat = torch.maximum(heat, (0.9 - 0.1 * k) * torch.exp(-((ys - cy) ** 2 + (xs - cx) ** 2).float() / 18.0))
    want = _check_centres(heat.unsqueeze(0), kernel, 20, cuda)
    assert want.shape[0] == 4


@pytest.mark.parametrize("shape,kernel", [pytest.param(shape, kernel, id="%d-shape%d" % (kernel, i))
                                          for kernel in (3, 7) for i, shape in enumerate([(64, 96), (37, 53)])]
                         + [pytest.param(ABOVE_256_WORKGROUPS, 3, id="3-above_256_workgroups")])
def test_centres_ties_at_the_cut(cuda, shape, kernel):
    """Eighths: the largest value is held by more than top_k pixels, all of them their window's maximum, so the
    top_k-th value is the largest one and nothing lies strictly above it."""
    g = torch.Generator().manual_seed(7)
    heat = torch.floor(torch.rand(1, *shape, generator=g) * 8) / 8
    assert int((heat == heat.max()).sum()) >= 200
    want = _check_centres(heat, kernel, 200, cuda)
    assert want.shape[0] == 0
    # a cut inside the value range: every pixel tied with the top_k-th value goes, so fewer than top_k - 1 stay
    sparse = heat * (torch.rand(1, *shape, generator=g) < 0.02)
    want = _check_centres(sparse, kernel, 5, cuda)
    assert want.shape[0] < 4


@pytest.mark.parametrize("shape", [(64, 96), (37, 53)])
def test_centres_below_threshold_and_plateau(cuda, shape):
    g = torch.Generator().manual_seed(3)
    assert _check_centres(torch.rand(1, *shape, generator=g) * 0.1, 7, 20, cuda).shape[0] == 0
    assert _check_centres(torch.full((1,) + shape, 0.5), 3, 5, cuda).shape[0] == 0


@pytest.mark.parametrize("shape", [(64, 96), (37, 53)])
@pytest.mark.parametrize("kernel", [3, 7])
def test_centres_on_border_and_corners(cuda, shape, kernel):
    h, w = shape
    g = torch.Generator().manual_seed(11)
    heat = torch.rand(1, h, w, generator=g) * 0.3
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h // 2, 0), (h - 1, w // 3), (h // 3, w - 1)]
    for k, (y, x) in enumerate(spots):
        heat[0, y, x] = 0.95 - 0.05 * k
    want = _check_centres(heat, kernel, 9, cuda)
    assert sorted(map(tuple, want.tolist())) == sorted(spots)


def test_centre_arguments(cuda):
    heat = torch.rand(1, 4, 5).to(cuda)
    with pytest.raises(RuntimeError):
        P.find_instance_center(heat, 0.1, 3, 21)            # more than H*W, as torch.topk
    with pytest.raises(NotImplementedError):
        P.find_instance_center(heat, 0.1, 3, None)


# ---- grouping ----------------------------------------------------------------------------------------------------------
def _distinct_centres(g, k, h, w):
    flat = torch.randperm(h * w, generator=g)[:k].sort().values
    return torch.stack([flat // w, flat % w], dim=1)


def test_grouping_exact_on_quarter_pixels(cuda):
    h, w, total_ties = 64, 128, 0
    for seed in (0, 1):
        g = torch.Generator().manual_seed(seed)
        centres = _distinct_centres(g, 40, h, w)
        offsets = torch.randint(-120, 121, (2, h, w), generator=g).float() / 4
        d = R.center_distances(centres, offsets).sort(dim=0).values
        total_ties += int((d[0] == d[1]).sum())
        want = R.group_pixels(centres, offsets)
        got = P.group_pixels(centres.to(cuda), offsets.to(cuda))
        assert got.dtype == torch.int64 and got.shape == (1, h, w)
        assert torch.equal(got.cpu(), want)
    assert total_ties > 0          # equal distances occur: the lowest centre index has to win them


def test_grouping_real_offsets(cuda):
    h, w = 64, 128
    g = torch.Generator().manual_seed(5)
    centres = _distinct_centres(g, 40, h, w)
    offsets = torch.randn(2, h, w, generator=g) * 20
    d64 = R.center_distances(centres, offsets, torch.float64)
    two = d64.sort(dim=0).values[:2]
    excused = ((two[1] - two[0]) < 1e-5 * two[1]).reshape(h, w)
    assert int(excused.sum()) <= 0.001 * h * w
    want = d64.argmin(dim=0).reshape(h, w) + 1
    got = P.group_pixels(centres.to(cuda), offsets.to(cuda)).cpu()[0]
    assert torch.equal(got[~excused], want[~excused])


def test_grouping_thing_mask_and_no_centre(cuda):
    h, w = 16, 70
    g = torch.Generator().manual_seed(6)
    offsets = (torch.randint(-20, 21, (2, h, w), generator=g).float() / 4).to(cuda)
    sem = torch.randint(0, 4, (h, w), generator=g, dtype=torch.int32).to(cuda)
    lut = P.thing_lut((1, 3), 4, cuda)
    centers = torch.tensor([[3, 4], [10, 60], [-1, -1]], dtype=torch.int32, device=cuda)
    two, none = torch.tensor([2], dtype=torch.int32, device=cuda), torch.tensor([0], dtype=torch.int32, device=cuda)
    free = P._group(centers, two, offsets)
    masked = P._group(centers, two, offsets, sem, lut)
    thing = (sem == 1) | (sem == 3)
    assert int(free.min()) == 1 and int(free.max()) == 2        # the unused third row is never a centre
    assert torch.equal(masked, free * thing.to(torch.int32))
    assert int(P._group(centers, none, offsets, sem, lut).abs().sum()) == 0


# ---- merge -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    z = np.load(GOLDEN)
    logits, heat, offsets = (torch.from_numpy(z[k]) for k in ("scene_logits", "scene_heat", "scene_offsets"))
    return dict(logits=logits, heat=heat, offsets=offsets, sem=logits.argmax(dim=0, keepdim=True),
                panoptic=torch.from_numpy(z["scene_panoptic"]), centers=torch.from_numpy(z["scene_centers"]))


def _scene_args():
    S = R.SCENE
    return (set(S["thing_ids"]), S["label_divisor"], S["stuff_area"], S["void_label"], S["threshold"], S["nms_kernel"],
            S["top_k"])


@pytest.mark.parametrize("id_offset", [0, 1])
def test_merge_scene(cuda, scene, id_offset):
    S = R.SCENE
    thing = R.thing_mask(scene["sem"], S["thing_ids"])
    centres = R.find_instance_center(scene["heat"].clone(), S["threshold"], S["nms_kernel"], S["top_k"])
    ins = thing * R.group_pixels(centres, scene["offsets"])
    want, rows = R.merge_semantic_and_instance(scene["sem"], ins, thing, S["label_divisor"], S["thing_ids"],
                                               S["stuff_area"], S["void_label"], id_offset)
    if id_offset == 0:
        assert torch.equal(want, scene["panoptic"].long())
    for mask in (thing.to(cuda), None):                      # the foreground mask given, or taken from the classes
        got, table = P.merge_semantic_and_instance(scene["sem"].to(cuda), ins.to(cuda), mask, S["label_divisor"],
                                                   S["thing_ids"], S["stuff_area"], S["void_label"], id_offset=id_offset,
                                                   num_classes=S["num_classes"], max_instances=S["top_k"],
                                                   return_table=True)
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
        assert table.dtype == torch.int32 and table.cpu().tolist() == rows
    void = S["void_label"] + id_offset
    assert int((want == void).sum()) > 0 and len(rows) == 7 and sum(r[1] for r in rows) == 5


def test_panoptic_surface_and_fused_form(cuda, scene):
    thing_ids, divisor, stuff_area, void, threshold, kernel, top_k = _scene_args()
    pan, centers = P.get_panoptic_segmentation(scene["sem"].to(cuda), scene["heat"].to(cuda), scene["offsets"].to(cuda),
                                               thing_ids, divisor, stuff_area, void, threshold, kernel, top_k)
    assert pan.dtype == torch.int64 and torch.equal(pan.cpu(), scene["panoptic"].long())
    assert torch.equal(centers.cpu(), scene["centers"].long())
    want, _, rows = R.get_panoptic_segmentation(scene["sem"], scene["heat"].clone(), scene["offsets"], thing_ids, divisor,
                                                stuff_area, void, threshold, kernel, top_k, id_offset=1)
    post = P.panoptic_deeplab_postprocess(scene["logits"].to(cuda), scene["heat"].to(cuda), scene["offsets"].to(cuda),
                                          thing_ids, divisor, stuff_area, threshold, kernel, top_k)
    assert post["panoptic"].dtype == torch.int32 and torch.equal(post["panoptic"].cpu().long(), want[0])
    assert post["table"].cpu().tolist() == rows == post["rows"]
    assert torch.equal(post["sem_seg"].cpu().long(), scene["sem"][0])
    assert int((post["panoptic"] == 0).sum()) > 0          # void is 0 with id_offset 1


def test_reference_defaults_with_a_small_label_divisor(cuda, scene):
    """top_k = 200 (the reference's default) with label_divisor 100: the centre buffer has more rows than the divisor,
    the five centres found do not."""
    thing_ids, divisor, stuff_area, void, threshold, kernel, _ = _scene_args()
    assert divisor < 200
    pan, centers = P.get_panoptic_segmentation(scene["sem"].to(cuda), scene["heat"].to(cuda), scene["offsets"].to(cuda),
                                               thing_ids, divisor, stuff_area, void, threshold, kernel, 200)
    assert torch.equal(pan.cpu(), scene["panoptic"].long()) and torch.equal(centers.cpu(), scene["centers"].long())
    ins, found = P.get_instance_segmentation(scene["sem"].to(cuda), scene["heat"].to(cuda), scene["offsets"].to(cuda),
                                             R.thing_mask(scene["sem"], thing_ids).to(cuda), thing_ids, threshold, kernel,
                                             200)
    want = R.thing_mask(scene["sem"], thing_ids) * R.group_pixels(scene["centers"][0].long(), scene["offsets"])
    assert torch.equal(found.cpu(), scene["centers"].long()) and torch.equal(ins.cpu(), want)
    quiet, none = P.get_instance_segmentation(scene["sem"].to(cuda), torch.zeros_like(scene["heat"]).to(cuda),
                                              scene["offsets"].to(cuda), R.thing_mask(scene["sem"], thing_ids).to(cuda),
                                              thing_ids, threshold, kernel, 200)
    assert none.shape == (1, 0, 2) and int(quiet.abs().sum()) == 0


def _merge_case(cuda, sem, ins, thing_ids, stuff_area=1, num_classes=6, max_instances=8, divisor=50):
    thing = R.thing_mask(sem, thing_ids)
    want, rows = R.merge_semantic_and_instance(sem, ins, thing, divisor, thing_ids, stuff_area, -1)
    got, table = P.merge_semantic_and_instance(sem.to(cuda), ins.to(cuda), thing.to(cuda), divisor, thing_ids, stuff_area,
                                               -1, num_classes=num_classes, max_instances=max_instances,
                                               return_table=True)
    assert torch.equal(got.cpu(), want) and table.cpu().tolist() == rows
    return want, rows


def test_merge_even_split_takes_the_smallest_class(cuda):
    sem = torch.zeros(1, 12, 70, dtype=torch.int64)
    sem[:, 2:8, 10:20] = 5
    sem[:, 2:8, 20:30] = 3                                   # instance 1: 60 pixels of class 5, 60 of class 3
    ins = torch.zeros_like(sem)
    ins[:, 2:8, 10:30] = 1
    _, rows = _merge_case(cuda, sem, ins, {3, 5})
    assert rows[0] == [3 * 50 + 1, 1, 3, 1, 120]


def test_merge_skips_instances_without_pixels(cuda):
    sem = torch.full((1, 9, 67), 1, dtype=torch.int64)
    sem[:, :, 5:60] = 4
    ins = torch.zeros_like(sem)
    ins[:, :, 5:20], ins[:, :, 20:40], ins[:, :, 40:60] = 1, 3, 6        # ids 2, 4, 5 won nothing
    want, rows = _merge_case(cuda, sem, ins, {4})
    assert [r[0] for r in rows] == [201, 202, 203, 50] and sorted(torch.unique(want).tolist()) == [50, 201, 202, 203]


def test_merge_without_centres_leaves_things_void(cuda, scene):
    thing_ids, divisor, stuff_area, void, threshold, kernel, top_k = _scene_args()
    quiet = torch.zeros_like(scene["heat"])
    want, centers, rows = R.get_panoptic_segmentation(scene["sem"], quiet.clone(), scene["offsets"], thing_ids, divisor,
                                                      stuff_area, void, threshold, kernel, top_k)
    assert centers.shape[1] == 0 and all(r[1] == 0 for r in rows)
    pan, got_centers = P.get_panoptic_segmentation(scene["sem"].to(cuda), quiet.to(cuda), scene["offsets"].to(cuda),
                                                   thing_ids, divisor, stuff_area, void, threshold, kernel, top_k)
    assert got_centers.shape == (1, 0, 2) and torch.equal(pan.cpu(), want)
    thing = R.thing_mask(scene["sem"], thing_ids) > 0
    assert bool((pan.cpu()[thing] == void).all())
    post = P.panoptic_deeplab_postprocess(scene["logits"].to(cuda), quiet.to(cuda), scene["offsets"].to(cuda), thing_ids,
                                          divisor, stuff_area, threshold, kernel, top_k)
    assert post["instances"].shape == (0, 8) and post["table"].cpu().tolist() == [[r[0] + 1] + r[1:] for r in rows]


# ---- instance rows -----------------------------------------------------------------------------------------------------
def test_instance_rows(cuda, scene):
    thing_ids, divisor, stuff_area, void, threshold, kernel, top_k = _scene_args()
    post = P.panoptic_deeplab_postprocess(scene["logits"].to(cuda), scene["heat"].to(cuda), scene["offsets"].to(cuda),
                                          thing_ids, divisor, stuff_area, threshold, kernel, top_k)
    pan, rows = post["panoptic"].cpu().long(), post["rows"]
    exact = R.instance_rows(pan, rows, scene["logits"], scene["heat"], torch.float64)
    stock = R.instance_rows(pan, rows, scene["logits"], scene["heat"], torch.float32)
    got = post["instances"].cpu().double()
    assert got.shape == exact.shape == (5, 8)
    assert torch.equal(got[:, :4], exact[:, :4]) and torch.equal(got[:, 6:], exact[:, 6:])     # boxes, centre pixel
    assert torch.equal(got[:, 5], exact[:, 5])                                               # the heat there
    stock_err = float((stock[:, 4] - exact[:, 4]).abs().max())
    err = float((got[:, 4] - exact[:, 4]).abs().max())
    print("semantic score: torch fp32 error %.3e, kernel error %.3e, bar %.3e" % (stock_err, err, 4 * stock_err))
    assert stock_err > 0 and err <= 4 * stock_err


def test_instance_rows_when_a_centre_wins_no_thing_pixel(cuda, scene):
    """A peak in a stuff stripe is a centre (the second in row-major order) whose pixels are all stuff: it takes no id
    and no row, and the rows of the later instances are still theirs."""
    thing_ids, divisor, stuff_area, void, threshold, kernel, top_k = _scene_args()
    heat = scene["heat"].clone()
    heat[0, 11, 30] = 0.97
    offsets = scene["offsets"].clone()
    offsets[:, 8:15, 27:34] = 0                             # the peak's neighbourhood (stuff) votes for itself
    want, centers, rows = R.get_panoptic_segmentation(scene["sem"], heat.clone(), offsets, thing_ids, divisor,
                                                      stuff_area, void, threshold, kernel, top_k, id_offset=1)
    assert centers.shape[1] == 6 and centers[0, 1].tolist() == [11, 30] and sum(r[1] for r in rows) == 5
    post = P.panoptic_deeplab_postprocess(scene["logits"].to(cuda), heat.to(cuda), offsets.to(cuda), thing_ids, divisor,
                                          stuff_area, threshold, kernel, top_k)
    assert int(post["num_centers"]) == 6 and post["rows"] == rows
    assert torch.equal(post["panoptic"].cpu().long(), want[0])
    exact = R.instance_rows(want, rows, scene["logits"], heat, torch.float64)
    got = post["instances"].cpu().double()
    assert torch.equal(got[:, :4], exact[:, :4]) and torch.equal(got[:, 5:], exact[:, 5:])
    stock = R.instance_rows(want, rows, scene["logits"], heat, torch.float32)
    assert float((got[:, 4] - exact[:, 4]).abs().max()) <= 4 * float((stock[:, 4] - exact[:, 4]).abs().max())


# ---- losses ------------------------------------------------------------------------------------------------------------
LOSSES = {"center": (P.center_loss, R.center_loss, 1), "offset": (P.offset_loss, R.offset_loss, 2)}


def _loss_inputs(kind, h, w, seed, scale=4, n=2):
    """pred as a [:, :c] slice of an 8-channel channels-last map (what conv2d_padded hands over); targets at least 0.5
    away from the up-sampled prediction, so that no |S p - t| is near a sign change."""
    c = LOSSES[kind][2]
    g = torch.Generator().manual_seed(seed)
    wide = torch.randn(n, 8, h, w, generator=g).contiguous(memory_format=CL)
    pred = wide[:, :c]
    up = torch.nn.functional.interpolate(pred.double(), scale_factor=scale, mode="bilinear", align_corners=False)
    up = up * (scale if kind == "offset" else 1)
    gap = (0.5 + 2.5 * torch.rand(up.shape, generator=g, dtype=torch.float64))
    gap = gap * (1 - 2 * (torch.rand(up.shape, generator=g) < 0.5).double())
    target = (up + gap).float()
    weights = (torch.rand(n, 1, h * scale, w * scale, generator=g) < 0.7).float()
    assert float((up - target.double()).abs().min()) >= 1e-4
    return wide, c, target, weights


def _device_loss(fn, wide, c, target, weights, scale, cuda):
    dev = wide.to(cuda).contiguous(memory_format=CL).requires_grad_(True)
    loss = fn(dev[:, :c], target.to(cuda), weights.to(cuda), scale)
    loss.backward()
    return loss.detach().cpu(), dev.grad.cpu()


@pytest.mark.parametrize("kind", ["center", "offset"])
@pytest.mark.parametrize("hw", [(8, 12), (1, 5), (5, 7), (19, 27, 16),       # (h, w) at stride 4, or (h, w, stride)
                                (5, 7, 3), (4, 3, 5), (3, 5, 6), (1, 2, 7)])
def test_losses(cuda, kind, hw):
    """(19, 27) at stride 16: 2 x 304 x 432 pixels are 342 chunks, so the finishing kernel folds two chunks per thread.
    Strides 3, 5, 6 and 7: 1 / stride is not exact in fp32, and the odd ones run the gather window's spare rows and columns."""
    fn, ref, _ = LOSSES[kind]
    scale = hw[2] if len(hw) > 2 else 4
    wide, c, target, weights = _loss_inputs(kind, hw[0], hw[1], seed=hw[0] * 10 + hw[1], scale=scale)
    pred = wide[:, :c]
    loss64, grad64 = R.loss_and_grad(ref, pred, target, weights, scale, torch.float64)
    loss32, grad32 = R.loss_and_grad(ref, pred, target, weights, scale, torch.float32)
    loss, grad = _device_loss(fn, wide, c, target, weights, scale, cuda)
    assert bool((grad[:, c:] == 0).all())                       # the padding channels get no gradient
    bar_l = 4 * float((loss32.double() - loss64).abs())
    bar_g = 4 * float((grad32.double() - grad64).abs().max())
    err_l = float((loss.double() - loss64).abs())
    err_g = float((grad[:, :c].double() - grad64).abs().max())
    print("%s %s: loss %.9g, error %.3e (bar %.3e); gradient error %.3e (bar %.3e)"
          % (kind, hw, float(loss64), err_l, bar_l, err_g, bar_g))
    assert bar_g > 0 and err_g <= bar_g
    assert err_l <= bar_l
    again, grad_again = _device_loss(fn, wide, c, target, weights, scale, cuda)
    assert torch.equal(again, loss) and torch.equal(grad_again, grad)


def test_offset_loss_sign_of_zero(cuda):
    pred = torch.zeros(2, 2, 5, 7, device=cuda, requires_grad=True)
    loss = P.offset_loss(pred, torch.zeros(2, 2, 20, 28, device=cuda), torch.ones(2, 1, 20, 28, device=cuda), 4)
    loss.backward()
    assert float(loss.detach()) == 0.0 and int((pred.grad != 0).sum()) == 0


@pytest.mark.parametrize("kind", ["center", "offset"])
def test_losses_with_zero_weights(cuda, kind):
    fn = LOSSES[kind][0]
    wide, c, target, weights = _loss_inputs(kind, 5, 7, seed=2)
    loss, grad = _device_loss(fn, wide, c, target, torch.zeros_like(weights), 4, cuda)
    assert float(loss) == 0.0 and int((grad != 0).sum()) == 0 and bool(torch.isfinite(grad).all())


def test_offset_weights_count_a_pixel_once(cuda):
    wide, c, target, weights = _loss_inputs("offset", 5, 7, seed=3)
    loss, _ = _device_loss(P.offset_loss, wide, c, target, weights, 4, cuda)
    per_channel = sum(float(R.offset_loss(wide[:, k:k + 1], target[:, k:k + 1], weights, 4)) for k in range(2))
    assert abs(float(loss) - per_channel) <= 1e-5 * per_channel


def test_loss_shapes_are_checked(cuda):
    pred = torch.zeros(1, 1, 4, 4, device=cuda)
    with pytest.raises(RuntimeError):
        P.center_loss(pred, torch.zeros(1, 1, 16, 12, device=cuda), torch.ones(1, 1, 16, 12, device=cuda), 4)
    with pytest.raises(ValueError):
        P.center_loss(pred, torch.zeros(1, 1, 10, 10, device=cuda), torch.ones(1, 1, 10, 10, device=cuda), 2.5)


# ---- Adam --------------------------------------------------------------------------------------------------------------
def _adam_setup(dtype, device, opt_cls):
    g = torch.Generator().manual_seed(9)
    shapes = [(3,), (5, 7), (2, 3, 3, 3), (1030,)]
    params = [torch.randn(*s, generator=g).to(dtype=dtype, device=device).requires_grad_(True) for s in shapes]
    grads = [[torch.randn(*s, generator=g) for s in shapes] for _ in range(3)]
    groups = [{"params": params[:2]}, {"params": params[2:], "weight_decay": 0.05, "lr": 2e-3}]
    return params, grads, opt_cls(groups, lr=1e-3)


def _adam_run(params, grads, opt, steps=3):
    for k in range(steps):
        for p, g in zip(params, grads[k]):
            p.grad = g.to(dtype=p.dtype, device=p.device)
        opt.step()
    return [p.detach().cpu().double() for p in params]


def test_adam_against_torch(cuda):
    from jtsm_amd.solver import Adam
    exact = _adam_run(*_adam_setup(torch.float64, "cpu", torch.optim.Adam))
    stock = _adam_run(*_adam_setup(torch.float32, "cpu", torch.optim.Adam))
    params, grads, opt = _adam_setup(torch.float32, cuda, Adam)
    got = _adam_run(params, grads, opt)
    stock_err = max(float((a - b).abs().max()) for a, b in zip(stock, exact))
    err = max(float((a - b).abs().max()) for a, b in zip(got, exact))
    print("Adam, three steps: torch fp32 error %.3e, kernel error %.3e, bar %.3e" % (stock_err, err, 4 * stock_err))
    assert stock_err > 0 and err <= 4 * stock_err
    st = opt.state[params[0]]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 3.0


def test_adam_takes_a_step_counter_from_the_device(cuda):
    """A checkpoint of a capturable / fused torch optimizer carries `step` on the device: it is brought to the host
    once and counts on from its value."""
    from jtsm_amd.solver import Adam
    params, grads, opt = _adam_setup(torch.float32, cuda, Adam)
    _adam_run(params, grads, opt, steps=1)
    twin_params, _, twin = _adam_setup(torch.float32, cuda, Adam)
    state = copy.deepcopy(opt.state_dict())
    for st in state["state"].values():
        st["step"] = st["step"].to(cuda)
    twin.load_state_dict(state)
    with torch.no_grad():
        for a, b in zip(twin_params, params):
            a.copy_(b)
    _adam_run(params, grads[1:], opt, steps=1)
    _adam_run(twin_params, grads[1:], twin, steps=1)
    st = twin.state[twin_params[0]]["step"]
    assert not st.is_cuda and float(st) == 2.0
    for a, b in zip(twin_params, params):
        assert torch.equal(a, b)


def test_adam_state_dict_round_trip(cuda):
    from jtsm_amd.solver import Adam
    params, grads, opt = _adam_setup(torch.float32, cuda, Adam)
    _adam_run(params, grads, opt, steps=2)
    # ours -> torch.optim.Adam -> ours, one more step on each side with the same gradient
    twins = [p.detach().clone().requires_grad_(True) for p in params]
    stock = torch.optim.Adam([{"params": twins[:2]}, {"params": twins[2:]}], lr=1.0)
    stock.load_state_dict(copy.deepcopy(opt.state_dict()))       # (a copy, as saving and loading makes one: torch hands
    #                                                               the `step` tensors over by reference)
    assert stock.param_groups[1]["weight_decay"] == 0.05 and stock.param_groups[1]["lr"] == 2e-3
    back_params = [p.detach().clone().requires_grad_(True) for p in params]
    back = Adam([{"params": back_params[:2]}, {"params": back_params[2:]}], lr=1.0)
    back.load_state_dict(copy.deepcopy(stock.state_dict()))
    for ps, o in ((params, opt), (twins, stock), (back_params, back)):
        for p, g in zip(ps, grads[2]):
            p.grad = g.to(cuda)
        o.step()
    for a, b, c in zip(params, twins, back_params):
        assert torch.equal(a, c)                                     # our state survives the trip bit for bit
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())
    assert float(stock.state[twins[0]]["step"]) == float(back.state[back_params[0]]["step"]) == 3.0
