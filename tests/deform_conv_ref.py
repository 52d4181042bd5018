"""Restatement of deformable convolution v1 / v2 (detectron2/layers/csrc/deformable/deform_conv_cuda_kernel.cu) that the
deformable tests are measured against.  A helper, not a test.  Two independent forms:

FORM 1 — NumPy, one Python loop step per (image, output pixel, tap, deformable group), the group's channels as a vector
whose elements each see exactly the reference's scalar arithmetic (every product and every sum rounded in `dtype`):
`columns`, `offset_mask_grad`, `input_grad`.  Arrays are channels-last, as the kernels take them: x (N, H, W, C), offset
(N, Ho, Wo, G * 2 * K), mask (N, Ho, Wo, G * K), cols / dcols (N * Ho * Wo, K, C).  In both dtypes the sampling
coordinate is first computed in float32 exactly as the kernel computes it — (float)(o * stride - pad + i * dil) + delta —
and then widened, so `floor` never differs between the float32 and the float64 run.

FORM 2 — vectorised torch (float64 in the tests) on logical NCHW tensors, gradients from autograd: `deform_conv_torch`.
"""
import os

import numpy as np
import torch


def out_size(size, k, stride, pad, dil):
    return (size + 2 * pad - dil * (k - 1) - 1) // stride + 1


class Frame(object):
    """Per (n, oy, ox, g, tap): the sampling point and its bilinear frame in `dtype`."""

    def __init__(self, offset, H, W, G, kh, kw, stride, pad, dil, dtype):
        N, Ho, Wo, ch = offset.shape
        K = kh * kw
        assert ch == G * 2 * K, (offset.shape, G, K)
        off = np.asarray(offset, dtype=np.float32).reshape(N, Ho, Wo, G, K, 2)
        i, j = np.arange(K) // kw, np.arange(K) % kw
        by = (np.arange(Ho)[:, None] * stride - pad + i[None, :] * dil).astype(np.float32)      # (Ho, K)
        bx = (np.arange(Wo)[:, None] * stride - pad + j[None, :] * dil).astype(np.float32)      # (Wo, K)
        h32 = by[None, :, None, None, :] + off[..., 0]
        w32 = bx[None, None, :, None, :] + off[..., 1]
        assert h32.dtype == np.float32 and w32.dtype == np.float32
        self.h, self.w = h32.astype(dtype), w32.astype(dtype)
        self.inside = (self.h > -1) & (self.w > -1) & (self.h < H) & (self.w < W)
        self.hl = np.floor(self.h).astype(np.int64)
        self.wl = np.floor(self.w).astype(np.int64)
        self.lh = self.h - self.hl.astype(dtype)
        self.lw = self.w - self.wl.astype(dtype)
        self.hh, self.hw = 1 - self.lh, 1 - self.lw
        assert self.lh.dtype == dtype and self.hh.dtype == dtype
        self.shape = (N, Ho, Wo, G, K)


def _units(shape):
    N, Ho, Wo, G, K = shape
    for n in range(N):
        for oy in range(Ho):
            for ox in range(Wo):
                for k in range(K):
                    for g in range(G):
                        yield n, oy, ox, g, k


def _corner_values(xn, hl, wl, H, W, sl, zero):
    """v1..v4 of deformable_im2col_bilinear: a corner is read only when it is in range."""
    hh_, wh_ = hl + 1, wl + 1
    v1 = xn[hl, wl, sl] if (hl >= 0 and wl >= 0) else zero
    v2 = xn[hl, wh_, sl] if (hl >= 0 and wh_ <= W - 1) else zero
    v3 = xn[hh_, wl, sl] if (hh_ <= H - 1 and wl >= 0) else zero
    v4 = xn[hh_, wh_, sl] if (hh_ <= H - 1 and wh_ <= W - 1) else zero
    return v1, v2, v3, v4


def _mask_of(mask, shape, dtype):
    N, Ho, Wo, G, K = shape
    if mask is None:
        return None
    return np.asarray(mask, dtype=dtype).reshape(N, Ho, Wo, G, K)


def columns(x, offset, mask, G, kh, kw, stride, pad, dil, dtype=np.float32):
    """cols (N Ho Wo, K, C) = mask * bilinear(x, p): deformable_im2col / modulated_deformable_im2col."""
    x = np.asarray(x, dtype=dtype)
    N, H, W, C = x.shape
    f = Frame(offset, H, W, G, kh, kw, stride, pad, dil, dtype)
    _, Ho, Wo, _, K = f.shape
    m = _mask_of(mask, f.shape, dtype)
    Cg = C // G
    cols = np.zeros((N * Ho * Wo, K, C), dtype=dtype)
    zero = np.zeros(Cg, dtype=dtype)
    for n, oy, ox, g, k in _units(f.shape):
        u = (n, oy, ox, g, k)
        if not f.inside[u]:
            continue
        sl = slice(g * Cg, (g + 1) * Cg)
        v1, v2, v3, v4 = _corner_values(x[n], f.hl[u], f.wl[u], H, W, sl, zero)
        hh, hw, lh, lw = f.hh[u], f.hw[u], f.lh[u], f.lw[u]
        w1, w2, w3, w4 = hh * hw, hh * lw, lh * hw, lh * lw
        val = w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4
        if m is not None:
            val = val * m[u]
        assert val.dtype == dtype
        cols[(n * Ho + oy) * Wo + ox, k, sl] = val
    return cols


def _ordered_sum(v):
    """Left-to-right sum in v's dtype (np.sum is pairwise)."""
    return np.add.accumulate(v)[-1] if v.size else v.dtype.type(0)


def offset_mask_grad(dcols, x, offset, mask, G, kh, kw, stride, pad, dil, dtype=np.float32):
    """d_offset (offset's layout), d_mask (mask's layout or None): deformable_col2im_coord /
    modulated_deformable_col2im_coord with get_coordinate_weight, channels summed in order."""
    x = np.asarray(x, dtype=dtype)
    dcols = np.asarray(dcols, dtype=dtype)
    N, H, W, C = x.shape
    f = Frame(offset, H, W, G, kh, kw, stride, pad, dil, dtype)
    _, Ho, Wo, _, K = f.shape
    m = _mask_of(mask, f.shape, dtype)
    Cg = C // G
    d_off = np.zeros((N, Ho, Wo, G, K, 2), dtype=dtype)
    d_mask = np.zeros((N, Ho, Wo, G, K), dtype=dtype) if m is not None else None
    zero = np.zeros(Cg, dtype=dtype)
    one = dtype(1)
    for n, oy, ox, g, k in _units(f.shape):
        u = (n, oy, ox, g, k)
        if not f.inside[u]:
            continue
        sl = slice(g * Cg, (g + 1) * Cg)
        hl, wl = f.hl[u], f.wl[u]
        v1, v2, v3, v4 = _corner_values(x[n], hl, wl, H, W, sl, zero)
        h, w = f.h[u], f.w[u]
        gh, gw = dtype(hl + 1) - h, dtype(wl + 1) - w          # (low + 1 - argmax)
        lh, lw = h - dtype(hl), w - dtype(wl)                  # (argmax - low)
        wy = zero + -one * gw * v1
        wy = wy + -one * lw * v2
        wy = wy + gw * v3
        wy = wy + lw * v4
        wx = zero + -one * gh * v1
        wx = wx + gh * v2
        wx = wx + -one * lh * v3
        wx = wx + lh * v4
        dc = dcols[(n * Ho + oy) * Wo + ox, k, sl]
        mm = m[u] if m is not None else one
        d_off[u + (0,)] = _ordered_sum(wy * dc * mm)
        d_off[u + (1,)] = _ordered_sum(wx * dc * mm)
        if m is not None:
            hh, hw = f.hh[u], f.hw[u]
            val = hh * hw * v1 + hh * f.lw[u] * v2 + f.lh[u] * hw * v3 + f.lh[u] * f.lw[u] * v4
            d_mask[u] = _ordered_sum(dc * val)
    d_off = d_off.reshape(N, Ho, Wo, G * 2 * K)
    return d_off, (d_mask.reshape(N, Ho, Wo, G * K) if m is not None else None)


def input_grad(dcols, offset, mask, x_shape, G, kh, kw, stride, pad, dil, dtype=np.float32):
    """dx (N, H, W, C): deformable_col2im / modulated_deformable_col2im with get_gradient_weight, the scatter taken in
    the order of the samples."""
    dcols = np.asarray(dcols, dtype=dtype)
    N, H, W, C = x_shape
    f = Frame(offset, H, W, G, kh, kw, stride, pad, dil, dtype)
    _, Ho, Wo, _, K = f.shape
    m = _mask_of(mask, f.shape, dtype)
    Cg = C // G
    dx = np.zeros((N, H, W, C), dtype=dtype)
    one = dtype(1)
    for n, oy, ox, g, k in _units(f.shape):
        u = (n, oy, ox, g, k)
        if not f.inside[u]:
            continue
        sl = slice(g * Cg, (g + 1) * Cg)
        h, w, hl, wl = f.h[u], f.w[u], f.hl[u], f.wl[u]
        top = dcols[(n * Ho + oy) * Wo + ox, k, sl]
        if m is not None:
            top = top * m[u]
        for y, xx in ((hl, wl), (hl, wl + 1), (hl + 1, wl), (hl + 1, wl + 1)):
            if not (0 <= y < H and 0 <= xx < W):
                continue
            wy = (dtype(y + 1) - h) if y == hl else ((h + one) - dtype(y))
            wx = (dtype(xx + 1) - w) if xx == wl else ((w + one) - dtype(xx))
            weight = wy * wx
            if weight != 0:
                dx[n, y, xx, sl] += weight * top
    return dx


# ---- form 2 ---------------------------------------------------------------------------------------------------------
def deform_columns_torch(x, offset, mask, kh, kw, stride, pad, dil, G):
    """(N, C, K, Ho * Wo) sampled columns of x (N, C, H, W) for offset (N, G * 2 * K, Ho, Wo), mask (N, G * K, Ho, Wo) or
    None; differentiable in x, offset and mask."""
    N, C, H, W = x.shape
    K = kh * kw
    Ho, Wo = out_size(H, kh, stride, pad, dil), out_size(W, kw, stride, pad, dil)
    assert offset.shape == (N, G * 2 * K, Ho, Wo), (offset.shape, (N, G * 2 * K, Ho, Wo))
    Cg = C // G
    off = offset.reshape(N, G, K, 2, Ho, Wo)
    k = torch.arange(K)
    i, j = torch.div(k, kw, rounding_mode="floor"), k % kw
    by = (torch.arange(Ho)[None, :] * stride - pad + i[:, None] * dil).to(x.dtype)      # (K, Ho)
    bx = (torch.arange(Wo)[None, :] * stride - pad + j[:, None] * dil).to(x.dtype)      # (K, Wo)
    h = by[None, None, :, :, None] + off[:, :, :, 0]
    w = bx[None, None, :, None, :] + off[:, :, :, 1]
    inside = (h > -1) & (w > -1) & (h < H) & (w < W)
    hl, wl = torch.floor(h).detach(), torch.floor(w).detach()
    lh, lw = h - hl, w - wl
    hh, hw = 1 - lh, 1 - lw
    flat = x.reshape(N, G, Cg, H * W)

    def corner(yy, xx):
        ok = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long().reshape(N, G, 1, K * Ho * Wo).expand(-1, -1, Cg, -1)
        v = torch.gather(flat, 3, idx).reshape(N, G, Cg, K, Ho, Wo)
        return v * ok.to(x.dtype)[:, :, None]

    val = (hh * hw)[:, :, None] * corner(hl, wl) + (hh * lw)[:, :, None] * corner(hl, wl + 1) + \
        (lh * hw)[:, :, None] * corner(hl + 1, wl) + (lh * lw)[:, :, None] * corner(hl + 1, wl + 1)
    if mask is not None:
        assert mask.shape == (N, G * K, Ho, Wo), mask.shape
        val = val * mask.reshape(N, G, 1, K, Ho, Wo)
    return val.reshape(N, C, K, Ho * Wo), (Ho, Wo)


def deform_conv_torch(x, offset, mask, weight, bias=None, stride=1, pad=0, dil=1, G=1):
    """y (N, O, Ho, Wo) of the (modulated) deformable convolution; weight (O, C, kh, kw)."""
    O, C, kh, kw = weight.shape
    cols, (Ho, Wo) = deform_columns_torch(x, offset, mask, kh, kw, stride, pad, dil, G)
    y = torch.einsum("ock,nckp->nop", weight.reshape(O, C, kh * kw), cols).reshape(x.shape[0], O, Ho, Wo)
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    return y


# ---- inputs -----------------------------------------------------------------------------------------------------------
def make_offsets(rng, N, Ho, Wo, G, K, span=4, integer_fraction=0.05):
    """Channels-last float32 offsets in [-span, span): an integer part plus a fraction that is a multiple of 2^-10 inside
    [2^-8, 1 - 2^-8] — every coordinate is exact in float32 and at least 1e-3 away from an integer — except for
    `integer_fraction` of the values, whose fraction is zero (exactly integer coordinates)."""
    shape = (N, Ho, Wo, G * 2 * K)
    whole = rng.integers(-span, span, size=shape)
    frac = rng.integers(4, 1021, size=shape) / 1024.0
    frac[rng.random(shape) < integer_fraction] = 0.0
    return (whole + frac).astype(np.float32)


def nhwc(t):
    """Logical NCHW torch tensor -> channels-last NumPy array."""
    return t.detach().permute(0, 2, 3, 1).contiguous().cpu().numpy()


def nchw(a, dtype=torch.float64):
    """Channels-last NumPy array -> logical NCHW torch tensor."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).permute(0, 3, 1, 2)


def rel_max(a, b):
    """max|a - b| / max|b| (the per-tensor criterion of tests/test_hip_conv.py)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if b.size else 0.0


# ---- the GPU cases ------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deform_reference_cases.npz")
SETTINGS = [(1, 1, 1), (2, 1, 1), (1, 2, 2), (2, 2, 2)]      # stride, pad, dil
SHAPES = [(2, 8, 2, 7, 9, 12), (1, 68, 1, 17, 19, 8), (2, 128, 4, 17, 19, 64)]      # N, C, G, H, W, O
OFFSET_UNIT = 1.0 / 1024     # the stored offsets are int16 multiples of this


def case_table():
    """(name, N, C, G, H, W, O, kh, kw, stride, pad, dil) of every GPU case; each runs as v1 and as v2 on the same offsets."""
    rows = []
    for si, (N, C, G, H, W, O) in enumerate(SHAPES):
        for stride, pad, dil in SETTINGS:
            rows.append(("s%d_%d%d%d" % (si, stride, pad, dil), N, C, G, H, W, O, 3, 3, stride, pad, dil))
    rows.append(("k1x1", 2, 8, 2, 7, 9, 12, 1, 1, 1, 0, 1))
    rows.append(("k3x1", 2, 8, 2, 7, 9, 12, 3, 1, 1, 1, 1))
    return rows


def offset_statistics(offset, H, W, G, kh, kw, stride, pad, dil):
    """(fraction of samples outside (-1, H) x (-1, W), fraction of exactly integer coordinates, smallest distance of
    the other coordinates to an integer)."""
    f = Frame(offset, H, W, G, kh, kw, stride, pad, dil, np.float64)
    coords = np.concatenate([f.h.ravel(), f.w.ravel()])
    dist = np.abs(coords - np.round(coords))
    exact = dist == 0
    return 1.0 - f.inside.mean(), exact.mean(), dist[~exact].min()


def case_inputs(row, seed):
    """(x, mask, dcols, weight, dy) of a case, channels-last float32 (weight (O, C, kh, kw), dy (N, O, Ho, Wo)): plain
    draws from the case's seed."""
    name, N, C, G, H, W, O, kh, kw, stride, pad, dil = row
    Ho, Wo = out_size(H, kh, stride, pad, dil), out_size(W, kw, stride, pad, dil)
    rng = np.random.default_rng(int(seed))
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    mask = rng.random((N, Ho, Wo, G * kh * kw)).astype(np.float32)
    dcols = rng.standard_normal((N * Ho * Wo, kh * kw, C)).astype(np.float32)
    weight = (rng.standard_normal((O, C, kh, kw)) / np.sqrt(C * kh * kw)).astype(np.float32)
    dy = rng.standard_normal((N, O, Ho, Wo)).astype(np.float32)
    return x, mask, dcols, weight, dy


def load_cases():
    """{name: (row, seed, offset float32 channels-last)} and the three reference errors of the golden file."""
    z = np.load(GOLDEN)
    cases = {}
    for row in case_table():
        name = row[0]
        cases[name] = (row, int(z[name + "_seed"]), z[name + "_offset"].astype(np.float32) * np.float32(OFFSET_UNIT))
    return cases, {k: float(z[k]) for k in ("T_ref_offset", "T_ref_mask", "T_ref_dx")}
