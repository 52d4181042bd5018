"""CPU suite: the two forms of tests/deform_conv_ref.py pin each other, and form 2 is pinned to F.conv2d by identities
(the reference's deformable code is device-only, so no reference binary can produce golden data)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deform_conv_ref as R

SETTINGS = [(1, 1, 1), (2, 1, 1), (1, 2, 2), (2, 2, 2)]     # stride, pad, dil


def _case(seed, N, C, G, H, W, O, kh, kw, stride, pad, dil, modulated):
    rng = np.random.default_rng(seed)
    Ho, Wo = R.out_size(H, kh, stride, pad, dil), R.out_size(W, kw, stride, pad, dil)
    x = rng.standard_normal((N, H, W, C))
    offset = R.make_offsets(rng, N, Ho, Wo, G, kh * kw)
    mask = rng.random((N, Ho, Wo, G * kh * kw)) if modulated else None
    weight = rng.standard_normal((O, C, kh, kw)) / np.sqrt(C * kh * kw)
    dy = rng.standard_normal((N, O, Ho, Wo))
    return x, offset, mask, weight, dy


@pytest.mark.parametrize("stride,pad,dil", SETTINGS)
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("modulated", [False, True])
def test_form1_fp64_equals_form2(modulated, G, stride, pad, dil):
    N, C, H, W, O, kh, kw = 2, 8, 7, 9, 4, 3, 3
    x, offset, mask, weight, dy = _case(7 + G, N, C, G, H, W, O, kh, kw, stride, pad, dil, modulated)
    K = kh * kw
    # form 2
    xt = R.nchw(x).requires_grad_()
    ot = R.nchw(offset).requires_grad_()
    mt = R.nchw(mask).requires_grad_() if modulated else None
    wt = torch.from_numpy(weight).requires_grad_()
    cols2, (Ho, Wo) = R.deform_columns_torch(xt, ot, mt, kh, kw, stride, pad, dil, G)
    y2 = R.deform_conv_torch(xt, ot, mt, wt, None, stride, pad, dil, G)
    grads = torch.autograd.grad(y2, [xt, ot, wt] + ([mt] if modulated else []), torch.from_numpy(dy))
    # form 1, float64
    cols1 = R.columns(x, offset, mask, G, kh, kw, stride, pad, dil, np.float64)            # (P, K, C)
    w_rows = weight.transpose(0, 2, 3, 1).reshape(O, K * C)                                # (O, K C): tap-major rows
    dy_rows = dy.transpose(0, 2, 3, 1).reshape(-1, O)
    y1 = (cols1.reshape(-1, K * C) @ w_rows.T).reshape(N, Ho, Wo, O)
    dcols = (dy_rows @ w_rows).reshape(-1, K, C)
    dw1 = (dy_rows.T @ cols1.reshape(-1, K * C)).reshape(O, kh, kw, C).transpose(0, 3, 1, 2)
    d_off1, d_mask1 = R.offset_mask_grad(dcols, x, offset, mask, G, kh, kw, stride, pad, dil, np.float64)
    dx1 = R.input_grad(dcols, offset, mask, x.shape, G, kh, kw, stride, pad, dil, np.float64)

    cols2 = cols2.detach().reshape(N, C, K, Ho * Wo).permute(0, 3, 2, 1).reshape(-1, K, C).numpy()
    assert R.rel_max(cols1, cols2) <= 1e-12
    assert R.rel_max(y1, R.nhwc(y2)) <= 1e-12
    assert R.rel_max(dx1, R.nhwc(grads[0])) <= 1e-12
    assert R.rel_max(d_off1, R.nhwc(grads[1])) <= 1e-12
    assert R.rel_max(dw1, grads[2].numpy()) <= 1e-12
    if modulated:
        assert R.rel_max(d_mask1, R.nhwc(grads[3])) <= 1e-12
    else:
        assert d_mask1 is None
    assert np.abs(d_off1).max() > 0 and np.abs(dx1).max() > 0


@pytest.mark.parametrize("stride,pad,dil", SETTINGS)
def test_zero_offsets_are_the_plain_convolution(stride, pad, dil):
    torch.manual_seed(0)
    N, C, H, W, O, G = 2, 8, 7, 9, 4, 2
    x = torch.randn(N, C, H, W, dtype=torch.float64)
    w = torch.randn(O, C, 3, 3, dtype=torch.float64)
    Ho, Wo = R.out_size(H, 3, stride, pad, dil), R.out_size(W, 3, stride, pad, dil)
    offset = torch.zeros(N, G * 18, Ho, Wo, dtype=torch.float64)
    want = F.conv2d(x, w, None, stride, pad, dil)
    for mask in (None, torch.ones(N, G * 9, Ho, Wo, dtype=torch.float64)):
        got = R.deform_conv_torch(x, offset, mask, w, None, stride, pad, dil, G)
        assert (got - want).abs().max().item() == 0.0


@pytest.mark.parametrize("stride,pad,dil", SETTINGS)
@pytest.mark.parametrize("dy,dx", [(1, -2), (-3, 2), (0, 4)])
def test_one_integer_offset_is_a_convolution_of_a_rebuilt_image(stride, pad, dil, dy, dx):
    """xp[y', x'] = x[y' - pad + dy, x' - pad + dx] (zero out of range), convolved with padding 0: a deformable sample
    that starts in the padding can land inside the image, so a shifted image convolved WITH padding is another function."""
    torch.manual_seed(1)
    N, C, H, W, O = 1, 4, 7, 9, 3
    x = torch.randn(N, C, H, W, dtype=torch.float64)
    w = torch.randn(O, C, 3, 3, dtype=torch.float64)
    Ho, Wo = R.out_size(H, 3, stride, pad, dil), R.out_size(W, 3, stride, pad, dil)
    offset = torch.zeros(N, 18, Ho, Wo, dtype=torch.float64)
    offset[:, 0::2] = dy
    offset[:, 1::2] = dx
    xp = torch.zeros(N, C, H + 2 * pad, W + 2 * pad, dtype=torch.float64)
    for yy in range(H + 2 * pad):
        for xx in range(W + 2 * pad):
            sy, sx = yy - pad + dy, xx - pad + dx
            if 0 <= sy < H and 0 <= sx < W:
                xp[:, :, yy, xx] = x[:, :, sy, sx]
    want = F.conv2d(xp, w, None, stride, 0, dil)
    got = R.deform_conv_torch(x, offset, None, w, None, stride, pad, dil, 1)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= 1e-13 * max(want.abs().max().item(), 1.0)


@pytest.mark.parametrize("modulated", [False, True])
def test_form2_passes_gradcheck(modulated):
    rng = np.random.default_rng(3)
    N, C, H, W, O, G = 1, 4, 7, 9, 2, 2
    x = torch.randn(N, C, H, W, dtype=torch.float64, requires_grad=True)
    w = torch.randn(O, C, 3, 3, dtype=torch.float64, requires_grad=True)
    offset = R.nchw(R.make_offsets(rng, N, H, W, G, 9, integer_fraction=0.0)).contiguous().requires_grad_()
    mask = torch.rand(N, G * 9, H, W, dtype=torch.float64, requires_grad=True) if modulated else None
    inputs = (x, offset, mask, w) if modulated else (x, offset, w)

    def fn(*a):
        if modulated:
            return R.deform_conv_torch(a[0], a[1], a[2], a[3], None, 1, 1, 1, G)
        return R.deform_conv_torch(a[0], a[1], None, a[2], None, 1, 1, 1, G)

    assert torch.autograd.gradcheck(fn, inputs, eps=1e-7, atol=1e-5)


def test_fp32_restatement_floors_like_fp64():
    """Both dtypes compute the coordinate in float32 first: the frames agree on floor and on inside."""
    rng = np.random.default_rng(5)
    offset = R.make_offsets(rng, 1, 7, 9, 1, 9)
    a = R.Frame(offset, 7, 9, 1, 3, 3, 1, 1, 1, np.float32)
    b = R.Frame(offset, 7, 9, 1, 3, 3, 1, 1, 1, np.float64)
    assert np.array_equal(a.hl, b.hl) and np.array_equal(a.wl, b.wl) and np.array_equal(a.inside, b.inside)
    assert np.array_equal(a.h.astype(np.float64), b.h)
