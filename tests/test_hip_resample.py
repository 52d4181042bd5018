"""GPU suite: the two resamplers that were only ever run behind a whole model — the bilinear xS up-sampler
(csrc/semseg_ops.hip: ups_fwd_kernel / ups_bwd_kernel, layers/elementwise.py: upsample_bilinear) and the nearest
resize of test-time augmentation (csrc/postprocess.hip: resize_nearest_kernel, layers/postprocess.py: resize_nearest).

upsample_bilinear against F.interpolate(mode="bilinear", align_corners=False) and its autograd in fp64 on the CPU, at
the scales whose reciprocal is not exact in fp32 (3, 5, 6, 7) next to the powers of two.  The bar is the project's one
for "the same arithmetic in another order of rounding": at most 4 x the error the same stock expression makes in fp32.
resize_nearest decides integers and copies: bit for bit against F.interpolate(mode="nearest") in fp32 on the CPU."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from jtsm_amd import _lib as L  # noqa: E402
from jtsm_amd.layers.elementwise import semseg_cross_entropy, upsample_bilinear, upsample_bilinear2x  # noqa: E402
from jtsm_amd.layers.postprocess import resize_nearest  # noqa: E402

CL = torch.channels_last
FULL_GRID = 8192 * 256            # items one launch covers before the grid-stride loop wraps (semseg_ops.hip: grid_for)


# ---- upsample_bilinear -------------------------------------------------------------------------------------------------
def _inputs(shape, scale, seed):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, c, h, w, generator=g), torch.randn(n, c, h * scale, w * scale, generator=g)


def _stock(x, gy, scale, dtype):
    """(F.interpolate(x), its input gradient under the upstream gradient gy) in `dtype` on the CPU."""
    xr = x.to(dtype, copy=True).requires_grad_(True)
    y = F.interpolate(xr, scale_factor=scale, mode="bilinear", align_corners=False)
    y.backward(gy.to(dtype))
    return y.detach(), xr.grad


def _device(x, gy, scale, layout, cuda):
    """(upsample_bilinear(x), the input gradient) from the device.  layout "cl": channels-last; "nchw": plain contiguous,
    which the wrapper re-lays out; "slice": the first channels of a channels-last map four channels wider."""
    if layout == "slice":
        wide = torch.cat([x, torch.full_like(x[:, :4], 7.0)], 1).to(cuda).contiguous(memory_format=CL).requires_grad_(True)
        xin = wide[:, :x.shape[1]]
        assert xin.stride(1) == 1 and not xin.is_contiguous(memory_format=CL)
        leaf = wide
    else:
        leaf = x.to(cuda)
        leaf = (leaf.contiguous() if layout == "nchw" else leaf.contiguous(memory_format=CL)).requires_grad_(True)
        xin = leaf
    y = upsample_bilinear(xin, scale)
    assert y.shape == gy.shape and y.is_contiguous(memory_format=CL)
    gd = gy.to(cuda)
    y.backward(gd.contiguous() if layout == "nchw" else gd.contiguous(memory_format=CL))
    torch.cuda.synchronize()
    grad = leaf.grad
    if layout == "slice":
        assert int((grad[:, x.shape[1]:] != 0).sum()) == 0       # the channels beside the slice get no gradient
        grad = grad[:, :x.shape[1]]
    return y.detach().cpu(), grad.cpu()


FP64_CASES = (
    [((2, 8, 5, 7), s, "cl") for s in (2, 3, 4, 5, 6, 7, 16)]
    # an axis of one source pixel: every tap along it clamps
    + [(shape, s, "cl") for shape in ((1, 4, 1, 5), (1, 4, 7, 1), (1, 4, 1, 1)) for s in (3, 4)]
    # 17 float4 chunks per pixel; 2550 outputs and 102 sources, so the last workgroup of either launch is ragged
    + [((1, 68, 3, 2), 5, "cl")]
    + [((2, 8, 5, 7), 3, "nchw"), ((2, 8, 5, 7), 5, "slice")])


@pytest.mark.parametrize("shape,scale,layout", FP64_CASES,
                         ids=["%s-x%d-%s" % ("x".join(map(str, sh)), s, lay) for sh, s, lay in FP64_CASES])
def test_upsample_bilinear_vs_fp64(cuda, shape, scale, layout):
    # (seeds at which the stock fp32 result is not exact anywhere: at 1 x 1 pixels and x3 it is, for about half the draws)
    x, gy = _inputs(shape, scale, seed=1000 * scale + sum(shape) + 2)
    y64, gx64 = _stock(x, gy, scale, torch.float64)
    y32, gx32 = _stock(x, gy, scale, torch.float32)
    y, gx = _device(x, gy, scale, layout, cuda)
    for what, got, w64, w32 in (("forward", y, y64, y32), ("input gradient", gx, gx64, gx32)):
        assert got.shape == w64.shape and got.dtype == torch.float32
        bar = 4 * float((w32.double() - w64).abs().max())
        err = float((got.double() - w64).abs().max())
        print("upsample_bilinear %s x%d %s, %s: error %.3e (bar %.3e)" % (shape, scale, layout, what, err, bar))
        assert bar > 0 and err <= bar, (what, err, bar)


@pytest.mark.parametrize("scale", [3, 4, 7])
def test_upsample_bilinear_backward_is_the_adjoint_of_the_forward(cuda, scale):
    """<up(x), g> = <x, up^T(g)>.  Forward and gather take their weights from one coordinate rule, so the two sides differ
    by the order of fp32 sums of at most (2 * scale)^2 terms only; each side is accumulated in fp64 from the device's
    fp32 outputs."""
    x, gy = _inputs((2, 8, 5, 7), scale, seed=40 + scale)
    y, gx = _device(x, gy, scale, "cl", cuda)
    lhs, rhs = float((y.double() * gy.double()).sum()), float((x.double() * gx.double()).sum())
    print("adjointness x%d: %.12g vs %.12g" % (scale, lhs, rhs))
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))


def test_upsample_bilinear_two_calls_give_identical_bits(cuda):
    x, gy = _inputs((2, 8, 5, 7), 5, seed=50)
    (y0, g0), (y1, g1) = (_device(x, gy, 5, "cl", cuda) for _ in range(2))
    assert torch.equal(y0, y1) and torch.equal(g0, g1)


def test_upsample_bilinear_scale_one_returns_the_input(cuda):
    x = torch.randn(1, 4, 3, 2, device=cuda)
    assert upsample_bilinear(x, 1) is x


@pytest.mark.parametrize("channels,scale,error", [(8, 2.5, ValueError), (8, 0, ValueError), (6, 3, RuntimeError)],
                         ids=["scale2.5", "scale0", "C6"])
def test_upsample_bilinear_refuses_before_it_launches(cuda, channels, scale, error):
    x = torch.randn(1, channels, 3, 2, device=cuda)
    L.TIMING = []                                                   # (records every library call while it is a list)
    try:
        with pytest.raises(error):
            upsample_bilinear(x, scale)
        assert L.TIMING == []                                       # no entry point was reached, so nothing was launched
    finally:
        L.TIMING = None


def test_upsample_bilinear_forward_past_one_full_grid(cuda):
    """64 channels of 24 x 24 at x16: 2 359 296 float4 outputs against the 2 097 152 a full grid covers in one pass, so
    the grid-stride loop takes a second one.  Once, against the stock fp32 result on the CPU: unit-normal inputs give
    rounding differences near 1e-6, and an output skipped or written from the wrong index is off by O(1)."""
    n, c, h, w, scale = 1, 64, 24, 24, 16
    assert n * (c // 4) * h * scale * w * scale > FULL_GRID
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(60))
    want = F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=False)
    y = upsample_bilinear(x.to(cuda).contiguous(memory_format=CL), scale).cpu()
    assert y.shape == want.shape
    assert float((y - want).abs().max()) <= 1e-5


def test_upsample_bilinear_backward_past_one_full_grid(cuda):
    """64 channels of 370 x 370 at x2: 2 190 400 float4 sources, so the gather's grid-stride loop takes a second pass.
    Compared with the composition, not with the CPU: upsample_bilinear2x's backward is the x2 kernel of the same
    definition, and both gradients stay on the device."""
    n, c, h, w = 1, 64, 370, 370
    assert n * (c // 4) * h * w > FULL_GRID
    gy = torch.randn(n, c, 2 * h, 2 * w, device=cuda, generator=torch.Generator(device=cuda).manual_seed(61))
    gy = gy.contiguous(memory_format=CL)
    grads = []
    for up in (lambda t: upsample_bilinear(t, 2), upsample_bilinear2x):
        x = torch.zeros(n, c, h, w, device=cuda).contiguous(memory_format=CL).requires_grad_(True)
        up(x).backward(gy)
        grads.append(x.grad)
    assert grads[0].shape == grads[1].shape == (n, c, h, w)
    assert float(grads[1].abs().max()) > 1.0                        # (the comparison is not of zeros)
    assert float((grads[0] - grads[1]).abs().max()) <= 1e-5


@pytest.mark.parametrize("scale", [3, 5])
def test_fused_cross_entropy_agrees_with_cross_entropy_of_upsample_bilinear(cuda, scale):
    """semseg_cross_entropy(z, t, S) and F.cross_entropy(upsample_bilinear(z, S), t), both on the device: the two
    up-sample by one coordinate rule, so a disagreement means one of them drifted.  The bar is test_hip_conv.py's
    `close` for the fused cross-entropy: 1e-4 of the largest reference value."""
    n, c, hs, ws = 2, 19, 4, 6
    g = torch.Generator().manual_seed(70 + scale)
    z = torch.randn(n, c, hs, ws, generator=g) * 3
    t = torch.randint(0, c, (n, hs * scale, ws * scale), generator=g)
    t[torch.rand(t.shape, generator=g) < 0.1] = 255
    td = t.to(cuda)
    zd = z.to(cuda).requires_grad_(True)
    fused = semseg_cross_entropy(zd, td, scale, 255)
    fused.backward()
    padded = torch.zeros(n, c + 1, hs, ws)                          # 20 channels: upsample_bilinear needs C % 4 == 0
    padded[:, :c] = z
    pd = padded.to(cuda).contiguous(memory_format=CL).requires_grad_(True)
    composed = F.cross_entropy(upsample_bilinear(pd, scale)[:, :c], td, reduction="mean", ignore_index=255)
    composed.backward()
    for what, a, b in (("loss", fused.detach(), composed.detach()), ("dlogits", zd.grad, pd.grad[:, :c])):
        a, b = a.cpu().double(), b.cpu().double()
        err, ref = float((a - b).abs().max()), float(b.abs().max())
        print("fused vs composed x%d, %s: error %.3e of %.3e" % (scale, what, err, ref))
        assert ref > 0 and err <= 1e-4 * ref, (what, err, ref)


# ---- resize_nearest ----------------------------------------------------------------------------------------------------
# (in, out) sizes of one axis: up, down, identity, from and to a single pixel ...
PLAIN = [(5, 13), (64, 37), (7, 7), (1, 9), (9, 1)]
# ... and pairs at which fp32 floor(o * (float(in) / out)), the rule of upsample_nearest2d, is not o * in // out
INEXACT = [(14, 46), (6, 74), (9, 111)]
PAIRS = PLAIN + INEXACT
# every pair on the rows with another on the columns, and the other way round; C in turn 1, 3, 54
NEAREST_CASES = ([((1, 3, 54)[i % 3], PAIRS[i], PAIRS[(i + 3) % 8]) for i in range(8)]
                 + [((3, 54, 1)[i % 3], PAIRS[(i + 6) % 8], PAIRS[i]) for i in range(8)]
                 + [(3, (8, 5), (100, 700))])                       # 700 columns: three workgroups to a row, the last ragged


def _nearest_cpu(x, out_hw, flip):
    return F.interpolate((x.flip(-1) if flip else x)[None], size=out_hw, mode="nearest")[0]


def test_the_inexact_pairs_are_inexact():
    """What the INEXACT pairs are listed for, established with stock torch alone."""
    for n_in, n_out in INEXACT:
        src = F.interpolate(torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in), size=(1, n_out), mode="nearest")
        exact = torch.arange(n_out) * n_in // n_out
        assert not torch.equal(src.view(-1).long(), exact), (n_in, n_out)


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "mirrored"])
@pytest.mark.parametrize("channels,rows,cols", NEAREST_CASES,
                         ids=["c%d-%dto%d-%dto%d" % (c, r[0], r[1], w[0], w[1]) for c, r, w in NEAREST_CASES])
def test_resize_nearest_bit_exact(cuda, channels, rows, cols, flip):
    g = torch.Generator().manual_seed(rows[0] * 1000 + cols[0])
    x = torch.randn(channels, rows[0], cols[0], generator=g)
    want = _nearest_cpu(x, (rows[1], cols[1]), flip)
    got = resize_nearest(x.to(cuda), (rows[1], cols[1]), flip_source=flip).cpu()
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(got, want), int((got != want).sum())


def test_resize_nearest_empty_output(cuda):
    x = torch.randn(3, 5, 7, device=cuda)
    for out_hw in ((0, 4), (6, 0), (0, 0)):
        y = resize_nearest(x, out_hw)
        assert y.shape == (3,) + out_hw and y.numel() == 0
    torch.cuda.synchronize()


def test_resize_nearest_refuses_more_rows_than_a_grid_has(cuda):
    x = torch.randn(1, 2, 2, device=cuda)
    with pytest.raises(RuntimeError, match="65535"):
        resize_nearest(x, (65536, 1))
    torch.cuda.synchronize()
    assert resize_nearest(x, (65535, 1)).shape == (1, 65535, 1)


@pytest.mark.parametrize("dtype", [torch.int64, torch.float16], ids=["int64", "fp16"])
def test_resize_nearest_converts_other_dtypes(cuda, dtype):
    g = torch.Generator().manual_seed(80)
    x = (torch.randint(-100, 100, (3, 14, 9), generator=g) if dtype == torch.int64
         else torch.randn(3, 14, 9, generator=g)).to(dtype)
    got = resize_nearest(x.to(cuda), (46, 5), flip_source=True)
    assert got.dtype == torch.float32
    assert torch.equal(got, resize_nearest(x.to(cuda).to(torch.float32), (46, 5), flip_source=True))
    assert torch.equal(got.cpu(), _nearest_cpu(x.to(torch.float32), (46, 5), True))
