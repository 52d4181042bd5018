"""GPU suite: the deformable-convolution kernels (csrc/deform_conv.hip) and the operator (jtsm_amd/layers/deform_conv.py)
against the restatement tests/deform_conv_ref.py, on the cases of tests/golden/deform_reference_cases.npz
(tests/golden/make_deform_golden.py).

* the columns are BIT-EQUAL to form 1 in float32;
* d_offset, d_mask and dx from given dcols lie within 4 x T_ref_* of form 1 in float64, T_ref_* being form 1's own
  float32-against-float64 error with the reference's sequential sums (recorded in the golden file).  The factor 4 covers
  the kernels' tree / list summation ORDER, not looser arithmetic;
* every kernel result is bit-identical across two calls, piled lists included;
* the whole operator against form 2 under the contraction criterion of tests/test_hip_conv.py: per tensor
  max|a - b| / max|b| <= 1e-4 and an element-wise allclose with rtol 1e-4 and atol 1e-4 max|b|, in the default and
  the f32 arithmetic.
"""
import functools
import importlib
import math

import numpy as np
import pytest
import torch

import deform_conv_ref as R

pytestmark = pytest.mark.gpu

from jtsm_amd.layers import DeformConv, ModulatedDeformConv, deform_conv, modulated_deform_conv  # noqa: E402
from jtsm_amd.layers import conv as K  # noqa: E402
from jtsm_amd.layers.batch_norm import FrozenBatchNorm2d  # noqa: E402

D = importlib.import_module("jtsm_amd.layers.deform_conv")     # (the package exports a function of that name)
CL = torch.channels_last
CASES, T_REF = R.load_cases()
NAMES = sorted(CASES)
REL = 1e-4


def dev(a, cuda):
    """Channels-last NumPy array -> logical NCHW device tensor in channels-last memory (the same bytes)."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda).permute(0, 3, 1, 2)


def host(t):
    """Logical NCHW device tensor -> channels-last NumPy array."""
    return t.detach().permute(0, 2, 3, 1).contiguous().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def geometry(row):
    name, N, C, G, H, W, O, kh, kw, stride, pad, dil = row
    return dict(kh=kh, kw=kw, stride=stride, pad=pad, dil=dil, G=G)


@functools.lru_cache(maxsize=None)
def reference(name, modulated):
    """Form 1 of one case, computed once: float32 columns, float64 gradients from the case's dcols."""
    row, seed, offset = CASES[name]
    _, N, C, G, H, W, O, kh, kw, stride, pad, dil = row
    x, mask, dcols, weight, dy = R.case_inputs(row, seed)
    m = mask if modulated else None
    args = (G, kh, kw, stride, pad, dil)
    cols32 = R.columns(x, offset, m, *args, np.float32)
    d_off, d_mask = R.offset_mask_grad(dcols, x, offset, m, *args, np.float64)
    dx = R.input_grad(dcols, offset, m, x.shape, *args, np.float64)
    return cols32, d_off, d_mask, dx


def close(a, b, what):
    """tests/test_hip_conv.py's criterion for a contraction."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    ref = np.abs(b).max() + 1e-30
    err = np.abs(a - b).max()
    print("%s: max err %.3e vs max ref %.3e (rel %.2e)" % (what, err, ref, err / ref))
    assert err <= REL * ref, "%s: max err %.3e vs max ref %.3e (rel %.2e)" % (what, err, ref, err / ref)
    assert np.allclose(a, b, rtol=REL, atol=REL * ref), what


@pytest.mark.parametrize("modulated", [False, True], ids=["v1", "v2"])
@pytest.mark.parametrize("name", NAMES)
def test_columns_are_bit_equal_to_the_float32_restatement(cuda, name, modulated):
    row, seed, offset = CASES[name]
    x, mask, dcols, weight, dy = R.case_inputs(row, seed)
    want = reference(name, modulated)[0]
    xd, od = dev(x, cuda), dev(offset, cuda)
    md = dev(mask, cuda) if modulated else None
    got = D.deform_columns(xd, od, md, **geometry(row))
    again = D.deform_columns(xd, od, md, **geometry(row))
    N, Ho, Wo = offset.shape[:3]
    g = host(got).reshape(want.shape)
    differ = np.flatnonzero(bits(g) != bits(want))
    assert differ.size == 0, "%d of %d words differ; first at %d: %r vs %r" % (
        differ.size, g.size, differ[0], g.ravel()[differ[0]], want.ravel()[differ[0]])
    assert torch.equal(got, again)
    assert np.abs(want).max() > 0


@pytest.mark.parametrize("modulated", [False, True], ids=["v1", "v2"])
@pytest.mark.parametrize("name", NAMES)
def test_gradient_kernels_against_the_float64_restatement(cuda, name, modulated):
    row, seed, offset = CASES[name]
    x, mask, dcols, weight, dy = R.case_inputs(row, seed)
    _, want_off, want_mask, want_dx = reference(name, modulated)
    N, Ho, Wo = offset.shape[:3]
    xd, od = dev(x, cuda), dev(offset, cuda)
    md = dev(mask, cuda) if modulated else None
    dc = dev(dcols.reshape(N, Ho, Wo, -1), cuda)
    geo = geometry(row)
    d_off, d_mask = D.deform_offset_mask_grad(dc, xd, od, md, **geo)
    d_off2, d_mask2 = D.deform_offset_mask_grad(dc, xd, od, md, **geo)
    dx = D.deform_input_grad(dc, od, md, xd.shape, **geo)
    dx2 = D.deform_input_grad(dc, od, md, xd.shape, **geo)
    e_off, e_dx = R.rel_max(host(d_off), want_off), R.rel_max(host(dx), want_dx)
    print("%s: d_offset %.3e (bound %.3e)  dx %.3e (bound %.3e)" % (name, e_off, 4 * T_REF["T_ref_offset"], e_dx,
                                                                  4 * T_REF["T_ref_dx"]))
    assert e_off <= 4 * T_REF["T_ref_offset"]
    assert e_dx <= 4 * T_REF["T_ref_dx"]
    if modulated:
        e_mask = R.rel_max(host(d_mask), want_mask)
        print("%s: d_mask %.3e (bound %.3e)" % (name, e_mask, 4 * T_REF["T_ref_mask"]))
        assert e_mask <= 4 * T_REF["T_ref_mask"]
        assert torch.equal(d_mask, d_mask2)
    else:
        assert d_mask is None
    assert torch.equal(d_off, d_off2) and torch.equal(dx, dx2)
    assert np.abs(want_off).max() > 0 and np.abs(want_dx).max() > 0


def _piled(kh, kw, pad, target):
    """Offsets that send every tap of every output pixel of a 17 x 19 map to `target`."""
    H, W = 17, 19
    Ho, Wo = R.out_size(H, kh, 1, pad, 1), R.out_size(W, kw, 1, pad, 1)
    K_ = kh * kw
    off = np.zeros((1, Ho, Wo, K_, 2), dtype=np.float32)
    i, j = np.arange(K_) // kw, np.arange(K_) % kw
    off[0, :, :, :, 0] = target[0] - (np.arange(Ho)[:, None, None] - pad + i[None, None, :])
    off[0, :, :, :, 1] = target[1] - (np.arange(Wo)[None, :, None] - pad + j[None, None, :])
    return off.reshape(1, Ho, Wo, 2 * K_), H, W, Ho, Wo


@pytest.mark.parametrize("kh,pad,target,longest", [(3, 1, (8.5, 9.25), 2907), (6, 3, (8.0, 9.0), 12960)],
                         ids=["four_lists_of_2907", "one_list_of_12960"])
def test_piled_lists_are_deterministic_and_right(cuda, kh, pad, target, longest):
    """Every sample lands on one pixel (3x3 taps at a fractional point: its four neighbours get 17 * 19 * 9 = 2907
    entries each, 11 628 in all; 6x6 taps at an integer point: ONE list of 18 * 20 * 36 = 12 960).  The lists are split
    over the slices of one workgroup and met by a tree: bit-identical across calls, and within the bound of that
    summation — ceil(L / slices) sequential additions, log2(slices) tree levels and three roundings per term, each at
    most 2^-24 of the sum of the terms' magnitudes (form 1 in float64 on |dcols| and |mask|)."""
    C, G = 8, 1
    offset, H, W, Ho, Wo = _piled(kh, kh, pad, target)
    rng = np.random.default_rng(11)
    K_ = kh * kh
    x = rng.standard_normal((1, H, W, C)).astype(np.float32)
    mask = rng.random((1, Ho, Wo, K_)).astype(np.float32)
    dcols = rng.standard_normal((Ho * Wo, K_, C)).astype(np.float32)
    geo = dict(kh=kh, kw=kh, stride=1, pad=pad, dil=1, G=G)
    args = (G, kh, kh, 1, pad, 1)
    want = R.input_grad(dcols, offset, mask, x.shape, *args, np.float64)
    size = R.input_grad(np.abs(dcols), offset, mask, x.shape, *args, np.float64)
    assert np.count_nonzero(np.abs(want).sum(-1)) in (1, 4)
    xd, od, md = dev(x, cuda), dev(offset, cuda), dev(mask, cuda)
    dc = dev(dcols.reshape(1, Ho, Wo, -1), cuda)
    dx = D.deform_input_grad(dc, od, md, xd.shape, **geo)
    dx2 = D.deform_input_grad(dc, od, md, xd.shape, **geo)
    assert torch.equal(dx, dx2)
    slices = 256 // 2          # C / G = 8: two lanes per list entry
    steps = math.ceil(longest / slices) + int(math.log2(slices)) + 3
    err = np.abs(host(dx).astype(np.float64) - want)
    print("piled: worst error / bound = %.3f" % (err / (steps * 2.0 ** -24 * size + 1e-300)).max())
    assert (err <= steps * 2.0 ** -24 * size).all()
    for fn in (lambda: D.deform_columns(xd, od, md, **geo), lambda: D.deform_offset_mask_grad(dc, xd, od, md, **geo)[0],
               lambda: D.deform_offset_mask_grad(dc, xd, od, md, **geo)[1]):
        assert torch.equal(fn(), fn())


@pytest.fixture(params=["default", "f32"])
def conv_math(request):
    old = K.MATH
    if request.param != "default":
        K.set_math(request.param)
    K.planes_clear()
    yield request.param
    K.set_math(old)
    K.planes_clear()


@pytest.mark.parametrize("modulated", [False, True], ids=["v1", "v2"])
@pytest.mark.parametrize("name", NAMES)
def test_operator_against_form2(cuda, conv_math, name, modulated):
    row, seed, offset = CASES[name]
    _, N, C, G, H, W, O, kh, kw, stride, pad, dil = row
    x, mask, dcols, weight, dy = R.case_inputs(row, seed)
    # form 2, float64 on the host
    xt, ot = R.nchw(x).requires_grad_(), R.nchw(offset).requires_grad_()
    mt = R.nchw(mask).requires_grad_() if modulated else None
    wt = torch.from_numpy(weight).double().requires_grad_()
    dyt = torch.from_numpy(dy).double()
    y2 = R.deform_conv_torch(xt, ot, mt, wt, None, stride, pad, dil, G)
    y2.backward(dyt)
    # the operator
    xd, od = dev(x, cuda).requires_grad_(), dev(offset, cuda).requires_grad_()
    md = dev(mask, cuda).requires_grad_() if modulated else None
    wd = torch.from_numpy(weight).to(cuda).contiguous(memory_format=CL).requires_grad_()
    if modulated:
        y = modulated_deform_conv(xd, od, md, wd, None, stride, pad, dil, 1, G)
    else:
        y = deform_conv(xd, od, wd, stride, pad, dil, 1, G)
    y.backward(torch.from_numpy(dy).to(cuda))
    close(y.detach().cpu(), y2.detach(), "y")
    close(xd.grad.cpu(), xt.grad, "dx")
    close(wd.grad.cpu(), wt.grad, "dw")
    close(od.grad.cpu(), ot.grad, "d_offset")
    if modulated:
        close(md.grad.cpu(), mt.grad, "d_mask")


@pytest.mark.parametrize("stride,pad,dil", R.SETTINGS)
def test_zero_offsets_agree_with_the_plain_convolution(cuda, conv_math, stride, pad, dil):
    torch.manual_seed(2)
    N, C, G, H, W, O = 2, 68, 1, 17, 19, 8
    x = torch.randn(N, C, H, W, device=cuda).contiguous(memory_format=CL)
    w = (torch.randn(O, C, 3, 3, device=cuda) / (C * 9) ** 0.5).contiguous(memory_format=CL)
    Ho, Wo = R.out_size(H, 3, stride, pad, dil), R.out_size(W, 3, stride, pad, dil)
    offset = torch.zeros(N, 18 * G, Ho, Wo, device=cuda)
    want = K.conv2d_fused(x, w, stride=stride, pad=pad, dil=dil)
    close(deform_conv(x, offset, w, stride, pad, dil, 1, G).cpu(), want.cpu(), "v1")
    ones = torch.ones(N, 9 * G, Ho, Wo, device=cuda)
    close(modulated_deform_conv(x, offset, ones, w, None, stride, pad, dil, 1, G).cpu(), want.cpu(), "v2")


def test_modules_fold_norm_bias_and_relu(cuda, conv_math):
    """ModulatedDeformConv(bias=True, norm=FrozenBN, activation=relu): one node, relu((conv + bias) * scale + shift);
    the bias gradient comes out of the weight-gradient contraction."""
    import torch.nn.functional as F

    row, seed, offset = CASES["s1_111"]
    _, N, C, G, H, W, O, kh, kw, stride, pad, dil = row
    x, mask, dcols, weight, dy = R.case_inputs(row, seed)
    torch.manual_seed(4)
    norm = FrozenBatchNorm2d(O)
    norm.weight.copy_(torch.rand(O) + 0.5)
    norm.bias.copy_(torch.randn(O))
    norm.running_mean.copy_(torch.randn(O) * 0.1)
    m = ModulatedDeformConv(C, O, 3, stride, pad, dil, 1, G, bias=True, norm=norm, activation=F.relu)
    with torch.no_grad():
        m.bias.copy_(torch.randn(O) * 0.3)
    scale, shift = (t.double() for t in norm.scale_bias())
    xt, ot, mt = R.nchw(x).requires_grad_(), R.nchw(offset).requires_grad_(), R.nchw(mask).requires_grad_()
    wt, bt = m.weight.detach().double().requires_grad_(), m.bias.detach().double().requires_grad_()
    y2 = torch.relu(R.deform_conv_torch(xt, ot, mt, wt, bt, stride, pad, dil, G) * scale.view(1, -1, 1, 1) +
                    shift.view(1, -1, 1, 1))
    y2.backward(torch.from_numpy(dy).double())
    m = m.to(cuda)
    assert m.weight.is_contiguous(memory_format=CL)
    xd, od, md = dev(x, cuda).requires_grad_(), dev(offset, cuda).requires_grad_(), dev(mask, cuda).requires_grad_()
    y = m(xd, od, md)
    y.backward(torch.from_numpy(dy).to(cuda))
    close(y.detach().cpu(), y2.detach(), "y")
    close(xd.grad.cpu(), xt.grad, "dx")
    close(m.weight.grad.cpu(), wt.grad, "dw")
    close(m.bias.grad.cpu(), bt.grad, "db")
    close(od.grad.cpu(), ot.grad, "d_offset")
    close(md.grad.cpu(), mt.grad, "d_mask")
    v1 = DeformConv(C, O, 3, stride, pad, dil, 1, G).to(cuda)
    assert "deformable_groups=1, bias=False" in repr(v1) and "bias=True" in repr(m)
    assert sorted(dict(v1.named_parameters())) == ["weight"]
    close(v1(xd.detach(), od.detach()).detach().cpu(),
          R.deform_conv_torch(xt.detach(), ot.detach(), None, v1.weight.detach().cpu().double(), None, stride, pad,
                              dil, G), "v1 module")


def test_batches_above_the_column_limit_loop_over_images(cuda, monkeypatch):
    row, seed, offset = CASES["s0_111"]
    _, N, C, G, H, W, O, kh, kw, stride, pad, dil = row
    x, mask, dcols, weight, dy = R.case_inputs(row, seed)

    def run():
        xd, od, md = dev(x, cuda).requires_grad_(), dev(offset, cuda).requires_grad_(), dev(mask, cuda).requires_grad_()
        wd = torch.from_numpy(weight).to(cuda).contiguous(memory_format=CL).requires_grad_()
        b = torch.zeros(O, device=cuda, requires_grad=True)
        y = modulated_deform_conv(xd, od, md, wd, b, stride, pad, dil, 1, G)
        y.backward(torch.from_numpy(dy).to(cuda))
        return [t.detach().cpu() for t in (y, xd.grad, od.grad, md.grad, wd.grad, b.grad)]

    whole = run()
    monkeypatch.setattr(D, "MAX_COLUMN_BYTES", 4 * 9 * C * 7 * 9)      # one image's columns
    for a, b, what in zip(run(), whole, ("y", "dx", "d_offset", "d_mask", "dw", "db")):
        close(a, b, what)


def test_empty_batch(cuda):
    m = DeformConv(8, 12, 3, 2, 1, 1).to(cuda)
    y = m(torch.zeros(0, 8, 7, 9, device=cuda), torch.zeros(0, 18, 4, 5, device=cuda))
    assert tuple(y.shape) == (0, 12, 4, 5)
    m2 = ModulatedDeformConv(8, 12, 3, 1, 1, 1, bias=True).to(cuda)
    y = m2(torch.zeros(0, 8, 7, 9, device=cuda), torch.zeros(0, 18, 7, 9, device=cuda), torch.zeros(0, 9, 7, 9, device=cuda))
    assert tuple(y.shape) == (0, 12, 7, 9)


def test_refusals(cuda):
    with pytest.raises(NotImplementedError):
        DeformConv(8, 8, 3, groups=2)
    with pytest.raises(NotImplementedError):
        ModulatedDeformConv(8, 8, 3, stride=(1, 2))
    with pytest.raises(NotImplementedError):
        DeformConv(8, 8, 3, padding=(1, 2))
    with pytest.raises(AssertionError):
        DeformConv(8, 8, 3, bias=True)
    x = torch.zeros(1, 8, 7, 9)
    w = torch.zeros(12, 8, 3, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        deform_conv(x, torch.zeros(1, 18, 7, 9), w, 1, 1, 1)
    xd, wd = x.to(cuda), w.to(cuda)
    with pytest.raises(NotImplementedError):
        deform_conv(xd, torch.zeros(1, 18, 7, 9, device=cuda), wd, 1, 1, 1, 2)
    with pytest.raises(NotImplementedError):
        deform_conv(xd, torch.zeros(1, 18, 7, 9, device=cuda), wd, 1, 1, (1, 2))
    with pytest.raises(ValueError, match=r"\(1, 20, 7, 9\).*\(1, 18, 7, 9\)"):
        deform_conv(xd, torch.zeros(1, 20, 7, 9, device=cuda), wd, 1, 1, 1)
    with pytest.raises(ValueError, match=r"\(1, 18, 7, 8\).*\(1, 18, 7, 9\)"):
        deform_conv(xd, torch.zeros(1, 18, 7, 8, device=cuda), wd, 1, 1, 1)
    with pytest.raises(ValueError, match=r"\(1, 9, 6, 9\).*\(1, 9, 7, 9\)"):
        modulated_deform_conv(xd, torch.zeros(1, 18, 7, 9, device=cuda), torch.zeros(1, 9, 6, 9, device=cuda), wd,
                              None, 1, 1, 1)
    with pytest.raises(ValueError, match=r"\(1, 18, 7, 9\).*\(1, 36, 7, 9\)"):      # two deformable groups want 36
        deform_conv(xd, torch.zeros(1, 18, 7, 9, device=cuda), wd, 1, 1, 1, 1, 2)
    with pytest.raises(RuntimeError, match="multiple of 4"):                        # C / G = 2
        deform_conv(xd, torch.zeros(1, 72, 7, 9, device=cuda), wd, 1, 1, 1, 1, 4)
