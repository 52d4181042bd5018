"""Every operand-plane producer against the definition, bit for bit (DESIGN.md "Operand planes").

A contraction in the bf16x3 / f16 arithmetics reads 16-bit planes INSTEAD of the fp32 tensor they were made from, so a
producer whose planes are not the split of the fp32 values it stored corrupts a training step silently — and by too
little for the end-to-end bars (1e-4 of the tensor's maximum) to see.  Here the expected words come from
tests/plane_ref.py (numpy integer arithmetic), applied to the fp32 tensor the SAME launch wrote wherever there is one,
and to the one CPU fp32 product where none is stored.  Comparison is array_equal on the 16-bit words.

Plane buffers are handed out pre-filled with a sentinel word, and every check also looks at the words between the
tensor's size and the buffer's rounded size: a tail that writes past n lands in the lo plane's neighbour."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import plane_ref as P

pytestmark = pytest.mark.gpu

from jtsm_amd import _lib as L  # noqa: E402
from jtsm_amd.layers import conv as K  # noqa: E402
from jtsm_amd.layers import elementwise as E  # noqa: E402
from test_hip_conv import CASES  # noqa: E402

CL = torch.channels_last
SENT = 0x5A5A
# body (8 per lane), the scalar tail of workgroup 0, one / several workgroups (2048 elements each)
SIZES = (1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049)
SIZES8 = (8, 64, 72, 2048, 2056, 4104)
# one full sweep of the split / relu / pass launchers' grid (8192 workgroups x 256 lanes x 8 elements) and a bit: the
# grid-stride loop takes a second trip, the tail still belongs to workgroup 0
SWEEP = 8192 * 256 * 8 + 2048 + 3
SWEEP8 = 8192 * 256 * 8 + 2056
SWEEP4 = 8192 * 256 * 4        # (the float4 kernels of elementwise.hip: grid_for caps at 8192 workgroups of 256 x 4)


@pytest.fixture(params=["bf16x3", "f16"])
def math(request, monkeypatch):
    old = K.MATH
    K.set_math(request.param)
    K.planes_clear()
    orig = K._planes_buf

    def sentinel_buf(n, device):
        return orig(n, device).fill_(SENT)

    monkeypatch.setattr(K, "_planes_buf", sentinel_buf)
    yield request.param
    K.set_math(old)
    K.planes_clear()


@pytest.fixture
def bf16x3(monkeypatch):
    old = K.MATH
    K.set_math("bf16x3")
    K.planes_clear()
    orig = K._planes_buf
    monkeypatch.setattr(K, "_planes_buf", lambda n, device: orig(n, device).fill_(SENT))
    yield
    K.set_math(old)
    K.planes_clear()


# ---- helpers --------------------------------------------------------------------------------------------------------
def memory_order(t):
    """The dense tensor's values in the order they lie in memory (what its planes mirror)."""
    t = t.detach()
    return torch.as_strided(t, (t.numel(),), (1,)).cpu().numpy()


def words(buf):
    return buf.detach().cpu().contiguous().numpy().view(np.uint16)


def same(got, want, what, x=None):
    if np.array_equal(got, want):
        return
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    rows = ["%d: x=%s got=%04x want=%04x" % (i, "?" if x is None else "%r(%08x)" % (float(x[i]), int(P.bits32(x[i:i + 1])[0])),
                                            int(got[i]), int(want[i])) for i in bad[:6]]
    pytest.fail("%s: %d of %d words differ (%.3f %%): %s" % (what, bad.size, got.size, 100.0 * bad.size / got.size,
                                                            "; ".join(rows)))


def expected(x, grad=False):
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    if K.MATH == "f16":
        return P.split_f16(x, K.GRAD_SHIFT if grad else 0), None
    return P.split_bf16(x)


def check_buf(buf, x, what, grad=False):
    """buf (layers/conv.py `_planes_buf`, unpaired) holds the planes of the fp32 values x — and nothing past them."""
    x = memory_order(x) if torch.is_tensor(x) else np.asarray(x, dtype=np.float32).reshape(-1)
    n = x.size
    w = words(buf)
    hi, lo = expected(x, grad)
    if K.MATH == "f16":
        same(w[:n], hi, what + " (fp16 plane)", x)
        rest = w[n:]
    else:
        n8 = w.size // 2
        same(w[:n], hi, what + " (hi)", x)
        same(w[n8:n8 + n], lo, what + " (lo)", x)
        rest = np.concatenate([w[n:n8], w[n8 + n:]])
    assert (rest == SENT).all(), "%s: %d words past the tensor's %d were written" % (what, int((rest != SENT).sum()), n)


def check_registered(t, what, grad=False):
    e = K._PLANES.get((t.data_ptr(), t.numel()))
    assert e is not None and e[1] == t._version, what + ": no planes were registered"
    check_buf(e[2], t, what, grad)


def vals(n, seed=0, shift=None, cap=None):
    """plane_ref.values; shift: keep the fp16 plane of x * 2^shift finite; cap: keep sums / products of a few finite."""
    x = P.values(n, seed, f16_shift=shift if K.MATH == "f16" else None)
    if cap is not None:
        x = np.where(np.abs(x) > cap, np.float32(1.0078125), x).astype(np.float32)
    return x


def dev(x, cuda):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


def mantissas(n, seed):
    """Factors in [0.5, 1.5) with random mantissas: a product with them is inexact on almost every element."""
    return (np.random.default_rng(seed).random(n) + 0.5).astype(np.float32)


# ---- the splits themselves ------------------------------------------------------------------------------------------
def _direct_split(x, cuda, shift):
    n = x.size
    src = dev(x, cuda)
    buf = K._planes_buf(n, cuda)
    hi, lo = K._hl(buf)
    if K.MATH == "f16":
        L.check(L.lib().jtsm_split_f16_f32(L.ptr(src), hi, n, shift, L.stream()), "split_f16")
        got = words(buf)
        same(got[:n], P.split_f16(x, shift), "split_f16 n=%d shift=%d" % (n, shift), x)
        assert (got[n:] == SENT).all(), ("split_f16 wrote past n", n)
    else:
        L.check(L.lib().jtsm_split_bf16_f32(L.ptr(src), hi, lo, n, L.stream()), "split_bf16")
        check_buf(buf, x, "split_bf16 n=%d" % n)


@pytest.mark.parametrize("n", [SIZES, SWEEP], ids=["small", "sweep"])
def test_split_kernels_by_direct_call(cuda, math, n):
    for k, m in enumerate(n if isinstance(n, tuple) else (n,)):
        shifts = (0,) if math == "bf16x3" else ((K.GRAD_SHIFT,) if m == SWEEP else (0, K.GRAD_SHIFT))
        for shift in shifts:
            _direct_split(vals(m, k, shift), cuda, shift)


def test_split_through_the_plane_cache(cuda, math):
    for k, (shape, grad) in enumerate([((2, 8, 3, 5), False), ((1, 24, 7, 9), True), ((3, 40), True), ((2049,), False)]):
        n = int(np.prod(shape))
        t = dev(vals(n, 10 + k, K.GRAD_SHIFT if grad else 0).reshape(shape), cuda)
        if t.dim() == 4:
            t = t.contiguous(memory_format=CL)
        check_buf(K.planes_of(t, grad=grad), t, "planes_of %s grad=%s" % (shape, grad), grad)
        assert K.planes_of(t, grad=grad) is K._PLANES[(t.data_ptr(), t.numel())][2]


def test_overflow_is_recorded(cuda, math):
    """Four elements whose plane overflows.  bf16: hi is +-inf, x - hi the other infinity (IEEE; the pair stands for
    NaN).  fp16: the plane word is +-inf from |x| * 2^shift >= 65520 on."""
    if math == "bf16x3":
        src = dev(P.OVERFLOW, cuda)
        buf = K._planes_buf(4, cuda)
        hi, lo = K._hl(buf)
        L.check(L.lib().jtsm_split_bf16_f32(L.ptr(src), hi, lo, 4, L.stream()), "split_bf16")
        w = words(buf)
        print("overflow words: hi", [hex(v) for v in w[:4]], "lo", [hex(v) for v in w[w.size // 2:w.size // 2 + 4]])
        assert list(w[:4]) == [0x7F80, 0xFF80, 0x7F80, 0xFF80]
        lo_w = w[w.size // 2:w.size // 2 + 4]
        assert ((lo_w & 0x7F80) == 0x7F80).all()                      # not finite: -+inf, or NaN with any payload
        assert np.isnan(P.plane_values(w[:4], lo_w)).all()
        return
    s = K.GRAD_SHIFT
    x = np.array([65520.0, -65520.0, 65536.0, 1e30], dtype=np.float32) * np.float32(2.0 ** -s)
    src = dev(np.concatenate([x, np.array([65519.996 * 2.0 ** -s] * 4, dtype=np.float32)]), cuda)
    buf = K._planes_buf(8, cuda)
    L.check(L.lib().jtsm_split_f16_f32(L.ptr(src), K._hl(buf)[0], 8, s, L.stream()), "split_f16")
    assert list(words(buf)[:8]) == [0x7C00, 0xFC00, 0x7C00, 0x7C00, 0x7BFF, 0x7BFF, 0x7BFF, 0x7BFF]


@pytest.mark.parametrize("k", [32, 64, 288, 1152])
def test_paired_split(cuda, bf16x3, k):
    for rows in (1, 3, 80):
        x = vals(rows * k, rows + k)
        buf = K._planes_buf(rows * k, cuda)
        L.check(L.lib().jtsm_split_bf16_paired_f32(L.ptr(dev(x, cuda)), L.ptr(buf), rows, k, L.stream()), "paired")
        hi, lo = P.split_bf16(x)
        w = words(buf)
        same(w[:2 * rows * k], P.paired(hi, lo, rows, k), "paired split rows=%d K=%d" % (rows, k))
        assert (w[2 * rows * k:] == SENT).all()


def _weight(o, i, taps, seed, cuda, shift=None):
    """A channels_last (o, i, kh, kw) weight over the value set (kept small enough to be scaled), and its [O][T][I] numpy."""
    kh = 3 if taps == 9 else 1
    w = vals(o * taps * i, seed, shift, cap=1e30).reshape(o, taps, i)
    t = dev(w, cuda).view(o, kh, taps // kh, i).permute(0, 3, 1, 2)
    assert t.permute(0, 2, 3, 1).is_contiguous()
    return t, w


TRANSPOSED = [(33, 8, 1), (80, 72, 9), (64, 64, 9), (256, 40, 1), (31, 33, 1)]


@pytest.mark.parametrize("shape", TRANSPOSED, ids=["%dx%dx%d" % s for s in TRANSPOSED])
def test_transposed_split(cuda, math, shape):
    o, i, taps = shape
    t, w = _weight(o, i, taps, o + i, cuda, shift=1)
    for scaled in (False, True):
        rs = mantissas(o, 3) if scaled else None
        rs_d = dev(rs, cuda) if scaled else None
        want = P.transposed(w, rs)                                   # [I][T][O]: ONE fp32 product, then the split
        buf = K._split_transposed(t, rs_d, paired=False)             # (the layout split_bf16_transposed returns)
        check_buf(buf, want, "transposed %s scaled=%s" % (shape, scaled))
        if math == "bf16x3":
            hi_v, lo_v = K.split_bf16_transposed(t, rs_d)
            hi, lo = P.split_bf16(want.reshape(-1))
            same(words(hi_v), hi, "split_bf16_transposed hi")
            same(words(lo_v), lo, "split_bf16_transposed lo")
        buf = K._weight_planes(t, True, rs_d)                        # (paired when the row length allows)
        if (taps * o) % 32 == 0 and math == "bf16x3":
            assert getattr(buf, "_paired", False)
            hi, lo = P.split_bf16(want)
            wd = words(buf)
            same(wd[:2 * want.size], P.paired(hi, lo, i, taps * o), "transposed paired %s scaled=%s" % (shape, scaled))
            assert (wd[2 * want.size:] == SENT).all()
        else:
            assert not getattr(buf, "_paired", False)
            check_buf(buf, want, "transposed via _weight_planes %s" % (shape,))


# ---- the table-driven re-split of every cached weight -----------------------------------------------------------------
TABLE_SHAPES = [(2, 4, 1), (23, 89, 1), (64, 32, 1), (8, 257, 1), (41, 100, 1), (48, 64, 9), (80, 256, 1), (8, 96, 9),
                (33, 8, 1), (31, 33, 1), (256, 40, 1), (16, 8, 9)]       # numel 8, 2047, 2048, 2056, 4100, ...


def _check_weight_buf(buf, want, rows, what):
    """`want`: the fp32 operand [rows][K] in its own order; buf paired or not as its flag says."""
    if getattr(buf, "_paired", False):
        hi, lo = P.split_bf16(want)
        wd = words(buf)
        same(wd[:2 * want.size], P.paired(hi, lo, rows, want.size // rows), what + " (paired)")
        assert (wd[2 * want.size:] == SENT).all(), what
    else:
        check_buf(buf, want, what)


@pytest.mark.parametrize("count", [1, 2, 150])
def test_weight_table_resplit(cuda, math, count):
    """refresh_weight_planes: ONE launch per form over a device table.  Every entry must hold the words of the
    single-launch producer and of the restatement — `find_entry` at every first_block boundary, entries of 1 and of
    several workgroups, with a ragged last one, paired and unpaired neighbours."""
    K._drop_planes()
    shapes = [TABLE_SHAPES[(k + (1 if count == 2 else 0)) % len(TABLE_SHAPES)] for k in range(count)]
    if count == 2:
        shapes = [(23, 89, 1), (8, 257, 1)]                              # 2047 then 2056: one block, then two
    params, scales = [], []
    for k, (o, i, taps) in enumerate(shapes):
        t, _ = _weight(o, i, taps, k, cuda, shift=1)
        params.append(torch.nn.Parameter(t.clone(memory_format=torch.preserve_format)))
        scales.append(dev(mantissas(o, 100 + k), cuda) if k % 3 else None)
        K._weight_planes(params[-1])                                     # (first use: the single-launch producers)
        K._weight_planes(params[-1], True, scales[-1])
    news = []
    with torch.no_grad():
        for k, (p, (o, i, taps)) in enumerate(zip(params, shapes)):
            t, w = _weight(o, i, taps, 1000 + k, cuda, shift=1)
            p.copy_(t)
            news.append(w)
    assert all(e.version != e.w._version for e in K._WPLANES.values())
    K.refresh_weight_planes()
    assert len(K._WTABLES) == 2 and all(e.version == e.w._version for e in K._WPLANES.values())
    for k, (p, w, rs, (o, i, taps)) in enumerate(zip(params, news, scales, shapes)):
        assert np.array_equal(memory_order(p), w.reshape(-1))
        what = "entry %d of %d %s" % (k, count, (o, i, taps))
        got = K._weight_planes(p)                                        # (cached: versions match, nothing is launched)
        _check_weight_buf(got, w.reshape(o, taps * i), o, what + " straight")
        single = K._weight_planes(p.detach().clone(memory_format=torch.preserve_format))
        assert torch.equal(got, single), what + " straight vs the single launch"
        got = K._weight_planes(p, True, rs)
        _check_weight_buf(got, P.transposed(w, None if rs is None else rs.cpu().numpy()), i, what + " transposed")
        single = K._weight_planes(p.detach().clone(memory_format=torch.preserve_format), True, rs)
        assert torch.equal(got, single), what + " transposed vs the single launch"
    K._drop_planes()


# ---- elementwise producers ------------------------------------------------------------------------------------------
def _gate(n, seed):
    """A ReLU output: +0, -0, positive subnormals, negatives, positives — the gate is y > 0."""
    rng = np.random.default_rng(seed)
    pool = np.array([0.0, -0.0, 2.0 ** -149, 2.0 ** -130, -2.0 ** -140, -1.0, 1.0, 3.5, 2.0 ** -126, -2.0 ** -126],
                    dtype=np.float32)
    return pool[rng.integers(0, pool.size, n)]


@pytest.mark.parametrize("n", [SIZES8, SWEEP8], ids=["small", "sweep"])
def test_relu_backward_planes(cuda, math, n):
    for k, m in enumerate(n if isinstance(n, tuple) else (n,)):
        dy, y = vals(m, 20 + k, K.GRAD_SHIFT), _gate(m, k)
        g = E.relu_backward(dev(dy, cuda), dev(y, cuda), emit_planes=True)
        same(P.bits32(memory_order(g)), P.bits32(np.where(y > 0, dy, np.float32(0))), "relu_backward g n=%d" % m)
        check_registered(g, "relu_backward n=%d" % m, grad=True)
    t = torch.zeros(12, device=cuda)                                     # n % 8 != 0: no planes, the next user splits
    g = E.relu_backward(t + 1, t + 1, emit_planes=True)
    assert (g.data_ptr(), 12) not in K._PLANES
    check_buf(K.planes_of(g, grad=True), g, "relu_backward n=12, split afresh", grad=True)


@pytest.mark.parametrize("scale", [1.0, 2.0, 1.0 / (1.0 - 0.3)])
def test_relu_backward_scaled_planes(cuda, math, scale):
    """kGateScaled: v = dy * scale in registers, g = v stored, planes of v.  The planes must be the split of the STORED
    g — a residual taken from a contracted multiply-subtract (the exact product's) differs on 1.6 % of lo words."""
    for k, m in enumerate(SIZES8 + ((SWEEP8,) if scale > 1.4 else ())):
        dy, y = vals(m, 30 + k, K.GRAD_SHIFT + 1, cap=1e30), _gate(m, k)
        g, buf = E.relu_backward_scaled(dev(dy, cuda), dev(y, cuda), scale)
        want = np.where(y > 0, dy * np.float32(scale), np.float32(0)).astype(np.float32)     # one IEEE product
        same(P.bits32(memory_order(g)), P.bits32(want), "relu_backward_scaled g n=%d" % m, dy)
        check_buf(buf, g, "relu_backward_scaled scale=%r n=%d" % (scale, m), grad=True)


# one element group, one wavefront's worth, and one element group past a full grid stride of the 8192-workgroup launch
@pytest.mark.parametrize("n", [8, 64, 8 * 256 * 8192 + 8])
def test_relu_backward_is_the_gate_at_scale_one(cuda, math, n):
    """kGate (dy passes through, no multiply) and kGateScaled at scale 1.0 are the same pass: the same g and the same
    plane words, bit for bit (-0, subnormals and huge values included), the sentinel words past the tensor too."""
    dy, y = dev(vals(n, 40, K.GRAD_SHIFT), cuda), dev(_gate(n, 7), cuda)
    g = E.relu_backward(dy, y, emit_planes=True)
    e = K._PLANES.get((g.data_ptr(), g.numel()))
    assert e is not None and e[1] == g._version, "relu_backward n=%d: no planes were registered" % n
    g1, buf1 = E.relu_backward_scaled(dy, y, 1.0)
    assert torch.equal(g.view(torch.int32), g1.view(torch.int32)), "n=%d: g differs" % n
    assert e[2].shape == buf1.shape and torch.equal(e[2], buf1), "n=%d: plane words differ" % n


@pytest.mark.parametrize("cols", [8, 16, 264])
def test_split_rowscale_planes(cuda, math, cols):
    """kRowScale stores no fp32 value: the expected operand is the one fp32 product, computed on the CPU.  cols = 8: the
    row factor changes with every 8-element group."""
    for k, rows in enumerate((1, 3, 257) + ((SWEEP8 // 8,) if cols == 8 and math == "bf16x3" else ())):
        x = vals(rows * cols, 40 + k, 1, cap=1e30).reshape(rows, cols)
        rs = mantissas(rows, k)
        buf = E.split_rowscale(dev(x, cuda), dev(rs, cuda))
        check_buf(buf, (x * rs[:, None]).astype(np.float32), "split_rowscale %dx%d" % (rows, cols))


@pytest.mark.parametrize("p", [0.0, 0.5, 0.3])
def test_dropout_split_planes(cuda, math, p):
    for k, m in enumerate(SIZES8):
        x = vals(m, 50 + k, 2, cap=1e30)
        y = dev(x, cuda)
        buf = E.dropout_split_(y, p, 1234 + k)
        got = memory_order(y)
        kept = np.float32(1.0) / (np.float32(1.0) - np.float32(p)) * x
        ok = (P.bits32(got) == P.bits32(kept.astype(np.float32))) | (P.bits32(got) == 0)
        assert ok.all(), "dropout: an element is neither x / (1 - p) nor +0"
        if p == 0.0:
            assert np.array_equal(P.bits32(got), P.bits32(x))
        check_buf(buf, y, "dropout_split_ p=%r n=%d" % (p, m))


def _cl_vals(shape, seed, cuda, cap=1e30):
    n, c, h, w = shape
    return dev(vals(n * c * h * w, seed, cap=cap).reshape(n, h, w, c), cuda).permute(0, 3, 1, 2)


@pytest.mark.parametrize("shape", [(1, 8, 2, 2), (2, 24, 6, 10), (1, 64, 2 * 182, 2 * 182)], ids=["tiny", "ragged", "sweep"])
def test_upsample2_add_planes(cuda, bf16x3, shape):
    n, c, h, w = shape
    assert shape[2] < 100 or n * c * h * w > SWEEP4           # (the last shape: more than one sweep of the grid)
    top, lat = _cl_vals((n, c, h // 2, w // 2), 1, cuda), _cl_vals(shape, 2, cuda)
    out = E.upsample2_add(top, lat)
    assert torch.equal(out, lat + torch.nn.functional.interpolate(top, scale_factor=2, mode="nearest"))
    check_registered(out, "upsample2_add %s" % (shape,))


@pytest.mark.parametrize("count", [2, 3, 4])
def test_sum_tensors_planes(cuda, bf16x3, count):
    for shape in ((1, 8, 1, 1), (2, 16, 5, 7), (1, 128, 3, 11)) + (((1, 64, 364, 364),) if count == 3 else ()):
        xs = [_cl_vals(shape, 60 + k, cuda) for k in range(count)]
        out = E.sum_tensors(xs)
        ref = xs[0]
        for x in xs[1:]:
            ref = ref + x
        assert torch.equal(out, ref), shape
        check_registered(out, "sum_tensors of %d %s" % (count, shape))


def test_narrow_maps_emit_no_planes_and_are_split_afresh(cuda, bf16x3):
    """C = 4: the float4 kernels could write planes, the wrappers must not (a consumer needs C % 8 == 0)."""
    xs = [_cl_vals((2, 4, 6, 6), 70 + k, cuda) for k in range(3)]
    for out in (E.sum_tensors(xs), E.upsample2_add(_cl_vals((2, 4, 3, 3), 9, cuda), xs[0])):
        assert (out.data_ptr(), out.numel()) not in K._PLANES
        check_buf(K.planes_of(out), out, "C = 4, split afresh")


@pytest.mark.parametrize("shape", [(1, 8, 1, 5), (1, 8, 7, 1), (2, 128, 16, 20)], ids=lambda s: "x".join(map(str, s)))
def test_upsample_bilinear2x_planes(cuda, bf16x3, shape):
    y = E.upsample_bilinear2x(_cl_vals(shape, 5, cuda, cap=1e4))
    assert tuple(y.shape) == (shape[0], shape[1], 2 * shape[2], 2 * shape[3])
    check_registered(y, "upsample_bilinear2x %s" % (shape,))


def test_group_norm_backward_planes(cuda, bf16x3):
    """group_norm_relu's backward registers the planes of dx (the output gradient of the convolution in front)."""
    g = torch.Generator().manual_seed(8)
    for shape, groups in (((2, 16, 5, 7), 4), ((1, 64, 9, 3), 16)):
        x = torch.randn(shape, generator=g).to(cuda).contiguous(memory_format=CL).requires_grad_(True)
        gamma, beta = (torch.rand(shape[1], generator=g) + 0.5).to(cuda), torch.randn(shape[1], generator=g).to(cuda)
        y = E.group_norm_relu(x, gamma, beta, groups)
        K._PLANES.clear()
        y.backward(torch.randn(shape, generator=g).to(cuda).contiguous(memory_format=CL))
        mine = [e for (ptr, n), e in K._PLANES.items() if n == x.numel()]
        assert len(mine) == 1
        check_buf(mine[0][2], mine[0][0], "group_norm backward dx %s" % (shape,))
        assert torch.equal(mine[0][0], x.grad)


# ---- contraction epilogues --------------------------------------------------------------------------------------------
EPILOGUE_NAMES = ("1x1", "3x3", "3x3_dil2", "ntail80", "ring_1x1", "ring_tail", "ring_3x3", "small_k")
EPILOGUE_CASES = [c for c in CASES if c[0] in EPILOGUE_NAMES] + [
    ("long_k",     2, 2048, 8, 8, 512, 1, 1, 0, 1),      # K = 2048 on few tiles: split over K
    ("halo_split", 2, 256, 32, 32, 256, 3, 1, 1, 1),     # the LDS-halo kernel, split over channel blocks
    ("wide_tail",  1, 64, 27, 27, 256, 1, 1, 0, 1),      # 729 rows: a row tail on every tile height
]


def _plan_row(case, role):
    _, n, c, h, w, o, k, s, p, d = case
    pl = K._plan((n, c, h, w), (o, c, k, k), s, p, d)
    if not pl.x3[role]:
        return None
    v = [C.c_int() for _ in range(6)]
    L.check(L.lib().jtsm_conv_bf16x3_plan(pl.ref, role, *[C.byref(x) for x in v]), "plan")
    wm, wn, tm, tn, nbuf, splits = [x.value for x in v]
    halo = nbuf == 0
    bm, bn = (16 * (16 if wm == 4 else 8), 32 * wn * tn) if halo else (32 * wm * tm, 32 * wn * tn)
    m = n * pl.oh * pl.ow if role == 0 else n * h * w
    return dict(case=case[0], role=("fwd", "dgrad")[role], kernel="halo" if halo else "generic", tile=(bm, bn),
                splits=splits, ring=nbuf > 2, halo=halo, row_tail=(not halo and m % bm != 0) or
                (halo and ((pl.oh if role == 0 else h) % (bm // 16) != 0 or (pl.ow if role == 0 else w) % 16 != 0)))


def test_epilogue_cases_reach_every_launch_class(cuda, math, capsys):
    """The shapes of test_contraction_epilogue_planes, per role: an unsplit launch, a split one (run there with either
    finishing mode), a 64x64-tile launch, a halo (3x3) launch and a launch with a row tail."""
    rows = [r for case in EPILOGUE_CASES for r in (_plan_row(case, 0), _plan_row(case, 1)) if r is not None]
    with capsys.disabled():
        print("\n%-11s %-6s %-8s %-10s %6s %5s %5s" % ("case", "role", "kernel", "tile", "slices", "ring", "tail"))
        for r in rows:
            print("%-11s %-6s %-8s %-10s %6d %5s %5s" % (r["case"], r["role"], r["kernel"], "%dx%d" % r["tile"],
                                                        r["splits"], r["ring"], r["row_tail"]))
    for role in ("fwd", "dgrad"):
        mine = [r for r in rows if r["role"] == role]
        assert any(r["splits"] == 1 for r in mine), role + ": no unsplit launch"
        assert any(r["splits"] > 1 for r in mine), role + ": no split launch"
        assert any(r["tile"] == (64, 64) for r in mine), role + ": no 64x64 tile"
        assert any(r["halo"] for r in mine), role + ": no halo launch"
        assert any(r["row_tail"] for r in mine), role + ": no row tail"


@pytest.fixture(params=[0, 1], ids=["separate_finish", "in_kernel_finish"])
def finish(request):
    L.lib().jtsm_conv_set_splitk_fused(request.param)
    yield request.param
    L.lib().jtsm_conv_set_splitk_fused(-1)


@pytest.mark.parametrize("case", EPILOGUE_CASES, ids=[c[0] for c in EPILOGUE_CASES])
def test_contraction_epilogue_planes(cuda, math, finish, case):
    """Planes written by a contraction's epilogue (put_planes: narrow / wide stores, the finishing pass, the in-kernel
    finish, the halo row map) = the split of the fp32 result of the SAME launch."""
    name, n, c, h, w, o, k, s, p, d = case
    pl = K._plan((n, c, h, w), (o, c, k, k), s, p, d)
    if not (pl.x3[0] or pl.x3[1]):
        assert name == "small_k"        # (8 channels under a 3x3 kernel: the one listed shape no plane role takes)
        return
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(n, c, h, w, generator=g).to(cuda).contiguous(memory_format=CL)
    wt = (torch.randn(o, c, k, k, generator=g) * (2.0 / (c * k * k)) ** 0.5).to(cuda).contiguous(memory_format=CL)
    sc, bi = dev(mantissas(o, 1), cuda), torch.randn(o, generator=g).to(cuda)
    oshape = (n, o, pl.oh, pl.ow)
    if pl.x3[0]:
        xp = K.PlaneTensor.of(x)
        res = torch.randn(oshape, generator=g).to(cuda).contiguous(memory_format=CL)
        y, yp = K.planes_forward(xp, wt, s, p, d, fp32="both")
        check_buf(yp.buf, y, name + " forward, plain")
        y, yp = K.planes_forward(xp, wt, s, p, d, fp32="both", scale=sc)
        check_buf(yp.buf, y, name + " forward, scale only")
        y, yp = K.planes_forward(xp, wt, s, p, d, bias=bi, relu=True, fp32="both", scale=sc, residual=res)
        check_buf(yp.buf, y, name + " forward, scale + bias + residual + relu")
        if math == "f16":
            y, yp = K.planes_forward(xp, wt, s, p, d, bias=bi, relu=True, fp32="both",
                                     residual_plane=K.PlaneTensor.of(res))
            check_buf(yp.buf, y, name + " forward, res16")
        y = K.conv2d_forward(x, wt, s, p, d, sc, bi, None, True, emit_planes=True)      # (the tensor front end)
        if o % 8 == 0:
            check_registered(y, name + " conv2d_forward(emit_planes)")
    if pl.x3[1]:
        dy = (torch.randn(oshape, generator=g) * 0.1).to(cuda).contiguous(memory_format=CL)
        gp = K.PlaneTensor.of(dy, grad=True)
        gate = K.PlaneTensor.of(torch.randn(n, c, h, w, generator=g).to(cuda).contiguous(memory_format=CL))
        xs = (n, c, h, w)
        dx, dp = K.planes_backward_data(gp, wt, xs, s, p, d, both=True)
        check_buf(dp.buf, dx, name + " dgrad, plain", grad=True)
        dx, dp = K.planes_backward_data(gp, wt, xs, s, p, d, gate=gate, kscale=sc, both=True)
        check_buf(dp.buf, dx, name + " dgrad, gate + kscale", grad=True)
        rs = dev(mantissas(n * h * w, 2), cuda)
        acc = (torch.randn(xs, generator=g) * 0.1).to(cuda).contiguous(memory_format=CL)
        dx, dp = K.planes_backward_data(gp, wt, xs, s, p, d, kscale=sc, row_scale=rs, accumulate=acc, both=True)
        check_buf(dp.buf, dx, name + " dgrad, row scale + accumulate", grad=True)
        if math == "f16":
            dx, dp = K.planes_backward_data(gp, wt, xs, s, p, d, gate=gate, both=True,
                                            accumulate_plane=K.PlaneTensor.of(acc, grad=True))
            check_buf(dp.buf, dx, name + " dgrad, acc16", grad=True)
        dx = K.conv2d_backward_data(dy, wt, xs, s, p, d, kscale=sc, relu_mask=x, emit_planes=True)
        if c % 8 == 0:
            check_registered(dx, name + " conv2d_backward_data(emit_planes)", grad=True)
        part = K._colsum_partials(pl, 1, c, cuda)
        if part is not None:
            dx = torch.empty(xs, dtype=torch.float32, device=cuda).contiguous(memory_format=CL)
            dp = K.PlaneTensor.empty(xs, cuda)
            K._launch_backward_data(pl, gp.buf, K._weight_planes(wt, True, None), dx, dp.buf, None, None, None,
                                    gate.buf, None, part)
            check_buf(dp.buf, dx, name + " dgrad, colsum", grad=True)


def test_conv_transpose_epilogue_planes(cuda, math, finish):
    g = torch.Generator().manual_seed(17)
    for (n, i, h, w, o) in ((2, 64, 6, 7, 32), (3, 256, 14, 14, 256)):
        x = torch.randn(n, i, h, w, generator=g).to(cuda).contiguous(memory_format=CL)
        wt = (torch.randn(i, o, 2, 2, generator=g) * 0.05).to(cuda).contiguous(memory_format=CL)
        bi = torch.randn(o, generator=g).to(cuda)
        y, yp = K.planes_conv_transpose2x2_forward(K.PlaneTensor.of(x), wt, bi, relu=True, fp32=True)
        check_buf(yp.buf, y, "conv_transpose forward %s" % ((n, i, h, w, o),))
        dy = (torch.randn(y.shape, generator=g) * 0.1).to(cuda).contiguous(memory_format=CL)
        dx = K.conv_transpose2x2_backward_data(dy, wt, relu_mask=x, emit_planes=True)
        check_registered(dx, "conv_transpose backward_data", grad=True)
        pl = K._plan(tuple(dy.shape), (i, o, 2, 2), 2, 0, 1)
        part = K._colsum_partials(pl, 0, i, cuda)
        if part is not None:
            dx = torch.empty((n, i, h, w), dtype=torch.float32, device=cuda).contiguous(memory_format=CL)
            dp = K.PlaneTensor.empty((n, i, h, w), cuda)
            K._launch_ct_backward_data(pl, K.planes_of(dy, grad=True), K._weight_planes(wt), dx, dp.buf,
                                       gate=K.planes_of(x), colsum=part)
            check_buf(dp.buf, dx, "conv_transpose backward_data, colsum", grad=True)


# ---- consumers of planes that are not contractions ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _csum_input(rows, ch, seed, f16):
    return P.values(rows * ch, seed, f16_shift=12 if f16 else None).reshape(rows, ch)


CSUM = [(1, 8), (37, 256), (300, 1024), (5000, 56)]


def _csum_check(got, pt, rows, ch, grad, what):
    w = words(pt.buf)
    n = rows * ch
    if K.MATH == "f16":
        v = P.plane_values(w[:n], None, K.GRAD_SHIFT if grad else 0)
    else:
        v = P.plane_values(w[:n], w[w.size // 2:w.size // 2 + n])
    v = v.reshape(rows, ch)
    ref, bar = v.sum(0), rows * 2.0 ** -24 * np.abs(v).sum(0)         # worst case of ANY fp32 summation order
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    assert (err <= bar).all(), "%s: %.3e over a bar of %.3e" % (what, float((err - bar).max()), float(bar[np.argmax(err - bar)]))


@pytest.mark.parametrize("shape", CSUM, ids=["%dx%d" % s for s in CSUM])
def test_planes_channel_sum(cuda, math, shape):
    rows, ch = shape
    x = dev(_csum_input(rows, ch, 3, math == "f16").reshape(rows, ch, 1, 1), cuda)
    for grad in (True, False):
        pt = K.PlaneTensor.of(x, grad=grad)
        got = K.planes_channel_sum(pt, grad=grad)
        _csum_check(got, pt, rows, ch, grad, "planes_channel_sum %s grad=%s" % (shape, grad))
        assert torch.equal(got, K.planes_channel_sum(pt, grad=grad))                  # reproducible bit for bit
        K.planes_clear()


@pytest.mark.parametrize("ch", [8, 256])
def test_planes_channel_sum_multi(cuda, math, ch):
    rows = (1, 37, 300, 5000, 64, 65, 2, 1000)
    pts = [K.PlaneTensor.of(dev(_csum_input(r, ch, 7 + k, math == "f16").reshape(r, ch, 1, 1), cuda), grad=True)
           for k, r in enumerate(rows)]
    got = K.planes_channel_sum_multi(pts)
    again = K.planes_channel_sum_multi(pts)
    for k, (r, pt) in enumerate(zip(rows, pts)):
        _csum_check(got[k], pt, r, ch, True, "planes_channel_sum_multi member %d (%d rows)" % (k, r))
        assert torch.equal(got[k], again[k])                                          # reproducible bit for bit
