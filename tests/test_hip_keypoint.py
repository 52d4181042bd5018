"""GPU suite: the keypoint kernels (jtsm_amd/csrc/keypoint.hip) against the NumPy restatement (tests/keypoint_ref.py)
and the vectors recorded from the reference (tests/golden/keypoint_reference_cases.npz): targets identical, loss and
gradient within the recorded loss bar, decode under the contract of test_keypoint_ref.check_decode, the head's tail
(4x4 transposed convolution + x2 bilinear) against fp64."""
import functools

import numpy as np
import pytest
import torch

import keypoint_ref as KR
from test_keypoint_ref import CASES, META, MK, check_decode, decode_case

pytestmark = pytest.mark.gpu

from jtsm_amd.layers import conv as CONV  # noqa: E402
from jtsm_amd.layers.keypoint import (keypoint_decode, keypoint_loss, keypoint_targets,  # noqa: E402
                                      keypoint_upsample)
from jtsm_amd.structures import Keypoints, heatmaps_to_keypoints  # noqa: E402

CL = torch.channels_last


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


# ---- targets --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MK.TARGET_CASES))
def test_targets_are_the_reference_integers(cuda, name):
    c = CASES[name]
    N, K, S = int(c["N"]), int(c["K"]), int(c["S"])
    kp, rois = MK.target_inputs(N, K, S, int(c["seed"]))
    t, v = Keypoints(dev(kp, cuda)).to_heatmap(dev(rois, cuda), S)
    assert t.dtype == torch.int32 and v.dtype == torch.uint8 and tuple(t.shape) == tuple(v.shape) == (N, K)
    assert np.array_equal(t.cpu().numpy(), c["targets"]) and np.array_equal(v.cpu().numpy(), c["valid"])


def test_targets_special_points(cuda):
    """x == x2 and y == y2 land in the last cell; cell edges x1 + j (x2 - x1) / S, points outside and v = 0 as the
    fp32 restatement has them (which equals the reference on the recorded cases)."""
    S = 56
    rois = np.array([[10.5, 20.25, 110.75, 75.5], [0, 0, 56, 56], [3.3, 4.4, 5.5, 9.9]], np.float32)
    kp = np.zeros((3, 60, 3), np.float32)
    for n, (x1, y1, x2, y2) in enumerate(rois):
        j = np.arange(60, dtype=np.float32)
        kp[n, :, 0] = x1 + j * (x2 - x1) / np.float32(S)
        kp[n, :, 1] = y1 + j[::-1] * (y2 - y1) / np.float32(S)
        kp[n, :, 2] = 1 + (np.arange(60) % 2)
        kp[n, 56, :2] = (x2, y2)
        kp[n, 57] = (x2, y1, 0)
    t, v = keypoint_targets(dev(kp, cuda), dev(rois, cuda), S)
    wt, wv = KR.keypoints_to_heatmap(kp, rois, S)
    assert np.array_equal(t.cpu().numpy(), wt) and np.array_equal(v.cpu().numpy(), wv)
    assert t[:, 56].tolist() == [S * S - 1] * 3 and v[:, 56].tolist() == [1] * 3 and v[:, 57].tolist() == [0] * 3
    assert not v[:, 58:].any()                      # j = 58, 59: beyond x2


# ---- loss -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loss_case(name):
    c = CASES[name]
    N, K, S = int(c["N"]), int(c["K"]), int(c["S"])
    logits, kp, rois = MK.loss_inputs(N, K, S, int(c["seed"]))
    t, v = KR.keypoints_to_heatmap(kp, rois, S)
    return logits, t, v, {norm: KR.keypoint_loss(logits, t, v, norm) for norm in (None, 37.5)}


@pytest.mark.parametrize("normalizer", [None, 37.5], ids=["visible", "fixed"])
@pytest.mark.parametrize("name", sorted(MK.LOSS_CASES))
def test_loss_and_gradient_against_fp64(cuda, name, normalizer):
    logits, t, v, want = loss_case(name)
    want_loss, want_grad = want[normalizer]
    x = dev(logits, cuda).requires_grad_()
    td, vd = dev(t.astype(np.int32), cuda), dev(v.astype(np.uint8), cuda)
    loss = keypoint_loss(x, td, vd, normalizer)
    (loss * 3.0).backward()
    bar = META["loss_bar"]
    got = float(loss.detach())
    print(name, normalizer, "loss", got, want_loss, "rel", abs(got - want_loss) / abs(want_loss))
    assert abs(got - want_loss) <= bar * abs(want_loss)
    g = x.grad.cpu().numpy().astype(np.float64) / 3.0
    worst = np.abs(g - want_grad).max() / np.abs(want_grad).max()
    print(name, normalizer, "grad rel", worst)
    assert worst <= bar
    # two runs give the same bits; the gradient buffer is fully written (the kernel is handed NaN-filled memory)
    x2 = dev(logits, cuda).requires_grad_()
    loss2 = keypoint_loss(x2, td, vd, normalizer)
    (loss2 * 3.0).backward()
    assert torch.equal(loss2.detach(), loss.detach()) and torch.equal(x2.grad, x.grad)


def test_loss_backward_writes_every_element(cuda):
    from jtsm_amd import _lib as L

    logits, t, v, want = loss_case("l3")
    N, K, S = logits.shape[:3]
    x, td, vd = dev(logits, cuda), dev(t.astype(np.int32), cuda), dev(v.astype(np.uint8), cuda)
    lib = L.lib()
    ws = torch.empty(lib.jtsm_keypoint_loss_workspace_bytes(N, K), dtype=torch.uint8, device=cuda)
    loss = torch.full((), float("nan"), device=cuda)
    L.check(lib.jtsm_keypoint_loss_forward_f32(L.ptr(x), L.ptr(td), L.ptr(vd), N, K, S, 0.0, L.ptr(loss), L.ptr(ws),
                                               L.stream()))
    grad = torch.full_like(x, float("nan"))
    one = torch.ones((), device=cuda)
    L.check(lib.jtsm_keypoint_loss_backward_f32(L.ptr(x), L.ptr(td), L.ptr(vd), N, K, S, L.ptr(one), L.ptr(ws),
                                                L.ptr(grad), L.stream()))
    assert bool(torch.isfinite(grad).all()) and not (v.reshape(-1) == 0).all()
    assert not grad.view(N * K, -1)[vd.view(-1) == 0].any()
    assert np.abs(grad.cpu().numpy() - want[None][1]).max() <= META["loss_bar"] * np.abs(want[None][1]).max()


@pytest.mark.parametrize("normalizer", [None, 8.0])
def test_loss_without_a_valid_row_is_exactly_zero(cuda, normalizer):
    x = (torch.randn(4, 3, 8, 8, device=cuda) * 3).requires_grad_()
    loss = keypoint_loss(x, torch.zeros(12, dtype=torch.int32, device=cuda), torch.zeros(12, dtype=torch.uint8, device=cuda),
                         normalizer)
    loss.backward()
    assert float(loss.detach()) == 0.0 and not x.grad.any() and bool(torch.isfinite(x.grad).all())


def test_loss_of_an_empty_batch(cuda):
    x = torch.zeros(0, 17, 56, 56, device=cuda, requires_grad=True)
    loss = keypoint_loss(x, torch.zeros(0, dtype=torch.int32, device=cuda), torch.zeros(0, dtype=torch.uint8, device=cuda))
    loss.backward()
    assert float(loss.detach()) == 0.0 and tuple(x.grad.shape) == (0, 17, 56, 56)


def test_loss_stays_finite_on_large_logits(cuda):
    rs = np.random.RandomState(5)
    logits = np.where(rs.uniform(size=(2, 3, 56, 56)) < 0.5, 80.0, -80.0).astype(np.float32)
    t = rs.randint(0, 56 * 56, (2, 3))
    v = np.ones((2, 3), np.int64)
    want, want_grad = KR.keypoint_loss(logits, t, v)
    x = dev(logits, cuda).requires_grad_()
    loss = keypoint_loss(x, dev(t.astype(np.int32), cuda), dev(v.astype(np.uint8), cuda))
    loss.backward()
    assert np.isfinite(float(loss)) and bool(torch.isfinite(x.grad).all())
    assert abs(float(loss) - want) <= META["loss_bar"] * abs(want)
    assert np.abs(x.grad.cpu().numpy() - want_grad).max() <= META["loss_bar"] * np.abs(want_grad).max()


# ---- decode ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MK.DECODE_CASES))
def test_decode_against_the_reference(cuda, name):
    maps, rois = decode_case(name)
    md, rd = dev(maps, cuda), dev(rois, cuda)
    before = md.clone()
    got = heatmaps_to_keypoints(md, rd)
    assert torch.equal(md, before)                      # the input is left as it was
    assert torch.equal(got, heatmaps_to_keypoints(md, rd))       # two runs, the same bits
    check_decode(got.cpu().numpy().astype(np.float64), name, maps, rois)


def test_decode_of_no_rois_and_of_a_constant_map(cuda):
    out = keypoint_decode(torch.zeros(0, 17, 56, 56, device=cuda), torch.zeros(0, 4, device=cuda))
    assert tuple(out.shape) == (0, 17, 4)
    # constant 0: every product and sum of the resize is exactly 0, so all pixels tie exactly and the lowest flat index
    # must win (another constant is not constant after the resize: the four coefficients sum to 1 only up to rounding)
    maps = torch.zeros((2, 3, 56, 56), device=cuda)
    rois = torch.tensor([[10.0, 20.0, 73.5, 141.25], [5.0, 6.0, 5.25, 6.5]], device=cuda)
    out = keypoint_decode(maps, rois).cpu().numpy()
    w, h, ow, oh, cx, cy = KR.roi_sizes(rois.cpu().numpy())
    # flat index 0: pixel (0, 0), whose centre is 0.5 corrected pixels from the corner
    assert np.array_equal(out[..., 0], np.broadcast_to((np.float32(0.5) * cx + rois.cpu().numpy()[:, 0])[:, None], (2, 3)))
    assert np.array_equal(out[..., 1], np.broadcast_to((np.float32(0.5) * cy + rois.cpu().numpy()[:, 1])[:, None], (2, 3)))
    assert not out[..., 2].any() and np.abs(out[..., 3] * 56 * 56 - 1).max() <= 1e-6
    assert ow.tolist() == [64, 1] and oh.tolist() == [122, 1]


# ---- the head's tail --------------------------------------------------------------------------------------------------
@pytest.fixture(params=["f32", "bf16x3"])
def conv_math(request):
    old = CONV.MATH
    CONV.set_math(request.param)
    CONV.planes_clear()
    yield request.param
    CONV.set_math(old)
    CONV.planes_clear()


@functools.lru_cache(maxsize=None)
def tail_case(R, C, K, H):
    rs = np.random.RandomState(R * 1000 + C + K + H)
    x = rs.standard_normal((R, C, H, H)).astype(np.float32)
    w = (rs.standard_normal((C, K, 4, 4)) / np.sqrt(4 * C)).astype(np.float32)
    b = rs.standard_normal(K).astype(np.float32)
    g = rs.standard_normal((R, K, 4 * H, 4 * H)).astype(np.float32)
    return x, w, b, g, KR.head_tail(x, w, b), KR.head_tail_grads(x, w, g)


@pytest.mark.parametrize("R,C,K,H", [(1, 32, 1, 2), (3, 32, 17, 14), (5, 64, 3, 7)])
def test_upsample_tail_against_fp64(cuda, conv_math, R, C, K, H):
    from jtsm_amd.modeling.roi_heads.keypoint_head import _ScoreLowres

    x, w, b, g, want, (dx, dw, db) = tail_case(R, C, K, H)
    layer = _ScoreLowres(C, K, 4, stride=2, padding=1).to(cuda)
    with torch.no_grad():
        layer.weight.copy_(dev(w, cuda))
        layer.bias.copy_(dev(b, cuda))
    xd = dev(x, cuda).contiguous(memory_format=CL).requires_grad_()
    out = keypoint_upsample(layer.parity_planes(xd), K)
    assert tuple(out.shape) == (R, K, 4 * H, 4 * H) and out.is_contiguous()
    out.backward(dev(g, cuda))
    torch.cuda.synchronize()
    fwd_bar, grad_bar = (1e-5, 1e-4) if conv_math == "f32" else (1e-3, 1e-3)

    def rel(a, ref):
        return float(np.abs(a.detach().cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max())

    errs = {"out": rel(out, want), "dx": rel(xd.grad, dx), "dw": rel(layer.weight.grad, dw), "db": rel(layer.bias.grad, db)}
    print(conv_math, (R, C, K, H), errs)
    assert errs["out"] <= fwd_bar and max(errs["dx"], errs["dw"], errs["db"]) <= grad_bar, errs
    # the shuffle alone (the module's own forward) is the transposed convolution
    low = layer(xd.detach())
    assert rel(low, KR.conv_transpose4x4(x, w, b)) <= fwd_bar


def test_upsample_backward_fills_the_padding_channels_with_zeros(cuda):
    R, K, H, W, Cp = 2, 3, 5, 6, 16
    z = torch.randn(R, Cp, H, W, device=cuda).contiguous(memory_format=CL).requires_grad_()
    out = keypoint_upsample(z, K)
    assert tuple(out.shape) == (R, K, 4 * H, 4 * W)
    g = torch.randn_like(out)
    out.backward(g)
    assert not z.grad[:, 4 * K:].any() and bool(torch.isfinite(z.grad).all())
    u = z.detach()[:, :4 * K].reshape(R, 2, 2, K, H, W).permute(0, 3, 4, 1, 5, 2).reshape(R, K, 2 * H, 2 * W)
    want = KR.bilinear_x2(u.cpu().numpy())
    assert np.abs(out.detach().cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()
    du = KR.bilinear_x2_grad(g.cpu().numpy())                                     # (R, K, 2H, 2W) -> parity planes
    dz = du.reshape(R, K, H, 2, W, 2).transpose(0, 3, 5, 1, 2, 4).reshape(R, 4 * K, H, W)
    assert np.abs(z.grad[:, :4 * K].cpu().numpy() - dz).max() <= 1e-5 * np.abs(dz).max()
    empty = keypoint_upsample(torch.zeros(0, Cp, H, W, device=cuda).contiguous(memory_format=CL), K)
    assert tuple(empty.shape) == (0, K, 4 * H, 4 * W)
