"""GPU suite (pytest -m gpu): ContextLocNet's ROILoopPool kernel (csrc/roi_loop_pool.hip) through the C ABI and the
jtsm_amd.layers / ROIPooler surfaces, against the CPU restatement of the CUDA contract (tests/roi_loop_pool_ref.py).

Bars: forward values and argmax bit-exact in both layouts; fp16 at the boundary exact; backward within 1e-6
(relative to the largest gradient) of the restatement's scatter-add, bit-identical across calls, bit-identical to the
float32 sum taken in the documented order, and unchanged by rois that name no image."""
import zlib

import numpy as np
import pytest
import torch

import roi_loop_pool_ref as ref
from test_roi_loop_pool_ref import FUSED_SPLIT_BOXES

pytestmark = pytest.mark.gpu

from jtsm_amd.layers import ROILoopPool  # noqa: E402
from jtsm_amd.layers.roi_loop_pool import roi_loop_pool_backward, roi_loop_pool_forward  # noqa: E402
from jtsm_amd.modeling.poolers import ROIPooler  # noqa: E402
from jtsm_amd.structures import Boxes  # noqa: E402

CL = torch.channels_last


def _rois(kind, rng, B, H, W, stride, R):
    """(R, 5) float32 rois in image coordinates of a (H*stride, W*stride) image."""
    ih, iw = H * stride, W * stride
    if kind in ("random", "stray"):
        xy = rng.uniform(0, [iw, ih], (R, 2))
        wh = rng.uniform(1, [iw / 2, ih / 2], (R, 2))
        boxes = np.concatenate([xy, xy + wh], 1)
    elif kind == "clustered":     # proposals piled on a few objects
        ctr = rng.uniform(0.2, 0.8, (4, 2)) * [iw, ih]
        c = ctr[rng.integers(0, 4, R)] + rng.normal(0, 8, (R, 2))
        wh = rng.uniform(16, [iw / 3, ih / 3], (R, 2))
        boxes = np.concatenate([c - wh / 2, c + wh / 2], 1)
    elif kind == "large":         # larger than the map
        c = rng.uniform(0, [iw, ih], (R, 2))
        wh = rng.uniform(iw, 3 * iw, (R, 2))
        boxes = np.concatenate([c - wh / 2, c + wh / 2], 1)
    elif kind == "borders":       # touching / crossing every border
        wh = rng.uniform(4, [iw / 2, ih / 2], (R, 2))
        side = rng.integers(0, 4, R)
        x0 = np.where(side == 0, rng.uniform(-20, 2, R), np.where(side == 1, iw - wh[:, 0] + rng.uniform(-2, 20, R),
                                                                  rng.uniform(0, iw - wh[:, 0], R)))
        y0 = np.where(side == 2, rng.uniform(-20, 2, R), np.where(side == 3, ih - wh[:, 1] + rng.uniform(-2, 20, R),
                                                                  rng.uniform(0, ih - wh[:, 1], R)))
        boxes = np.stack([x0, y0, x0 + wh[:, 0], y0 + wh[:, 1]], 1)
    elif kind == "degenerate":    # zero / negative extent, sub-cell boxes
        xy = rng.uniform(0, [iw, ih], (R, 2))
        wh = rng.uniform(-stride, stride / 2, (R, 2))
        boxes = np.concatenate([xy, xy + wh], 1)
    else:
        raise ValueError(kind)
    b = rng.integers(0, B, (R, 1))
    if kind == "stray":           # ordinary boxes, a quarter of them naming no image: -1 and B in turn
        b[1::4, 0] = np.where(np.arange(len(b[1::4])) % 2 == 0, -1, B)
    return np.concatenate([b, boxes], 1).astype(np.float32)


def _sum_in_order(arg, g, b, B, C, H, W):
    """float32 scatter-add in the order given: row i of arg / g (N, C) adds g[i, c] to cell arg[i, c] of image b[i],
    channel c, where arg >= 0 and b names an image.  np.add.at adds sequentially in index order (rows, then channels),
    so per (cell, channel) the terms are added in row order, starting from 0 — as the gather kernels do."""
    gin = np.zeros((B, C, H * W), np.float32)
    bb = np.broadcast_to(b.astype(np.int64)[:, None], arg.shape)
    cc = np.broadcast_to(np.arange(C)[None], arg.shape)
    ok = (arg >= 0) & (bb >= 0) & (bb < B)
    np.add.at(gin, (bb[ok], cc[ok], arg[ok]), g[ok].astype(np.float32))
    return gin.reshape(B, C, H, W)


def _rows(t, R):
    """(R, C, PH, PW) -> (R, PH * PW, C): a roi's bins in ph-outer / pw-inner order."""
    return t.transpose(0, 2, 3, 1).reshape(R, -1, t.shape[1])


def _feat(rng, B, C, H, W, kind="relu"):
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    if kind == "relu":            # post-ReLU features: zeros and ties included
        return np.maximum(x, 0)
    if kind == "zero":
        return np.zeros_like(x)
    if kind == "negative":
        return -np.abs(x) - 0.5
    return x


def _gpu_forward(x, rois, scale, P, cuda, nhwc):
    xt = torch.from_numpy(x).to(cuda)
    if nhwc:
        xt = xt.contiguous(memory_format=CL)
    out, arg = roi_loop_pool_forward(xt, torch.from_numpy(rois).to(cuda), scale, P, P)
    if nhwc and out.numel():
        assert out.is_contiguous(memory_format=CL) and arg.is_contiguous(memory_format=CL)
    return out.cpu().numpy(), arg.cpu().numpy()


CASES = [("random", "relu", 1, 16, 48), ("clustered", "relu", 2, 64, 60), ("large", "relu", 2, 8, 20),
         ("borders", "relu", 2, 12, 40), ("degenerate", "relu", 1, 8, 30), ("random", "zero", 2, 8, 10),
         ("random", "negative", 1, 4, 10), ("clustered", "signed", 3, 3, 25), ("random", "relu", 2, 8, 0),
         ("stray", "relu", 2, 8, 40)]


@pytest.mark.parametrize("nhwc", [True, False], ids=["nhwc", "nchw"])
@pytest.mark.parametrize("kind,feat,B,C,R", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_forward_matches_restatement_bit_exact(cuda, kind, feat, B, C, R, nhwc):
    rng = np.random.default_rng(zlib.crc32(repr((kind, feat, B, C, R)).encode()))
    H, W, stride, P = 20, 24, 8, 7
    x = _feat(rng, B, C, H, W, feat)
    rois = _rois(kind, rng, B, H, W, stride, R)
    want, want_arg = ref.forward(x, rois, 1.0 / stride, P, P)
    got, got_arg = _gpu_forward(x, rois, 1.0 / stride, P, cuda, nhwc)
    assert got.shape == (3 * R, C, P, P)
    np.testing.assert_array_equal(got_arg, want_arg)
    np.testing.assert_array_equal(got, want)
    if kind == "stray":           # a roi naming no image pools nothing, in all three blocks
        bad = np.tile((rois[:, 0] < 0) | (rois[:, 0] >= B), 3)
        assert bad.sum() == 3 * 10 and (got[bad] == 0).all() and (got_arg[bad] == -1).all()
        assert (got_arg[~bad] >= 0).any()


def test_forward_unfused_reading_on_the_split_boxes(cuda):
    """The listed boxes on which a contracted `w*1.8f - w` would round the outer rectangle differently: the kernel
    follows the unfused reading, as the restatement does."""
    rng = np.random.default_rng(7)
    x = _feat(rng, 1, 8, 128, 128)
    rois = np.array([(0,) + b for b, _, _ in FUSED_SPLIT_BOXES], np.float32)
    want, want_arg = ref.forward(x, rois, 0.125, 7, 7)
    for nhwc in (True, False):
        got, got_arg = _gpu_forward(x, rois, 0.125, 7, cuda, nhwc)
        np.testing.assert_array_equal(got_arg, want_arg)
        np.testing.assert_array_equal(got, want)
    fused, _ = ref.forward(x, rois, 0.125, 7, 7, fused=True)
    assert not np.array_equal(fused, want)     # (the listed boxes do reach the pooled values)


def test_forward_flagship_channels(cuda):
    """512 channels (the shipped config's res5), channels-last: the 16-byte-per-lane path, two channel blocks."""
    rng = np.random.default_rng(11)
    B, C, H, W = 2, 512, 24, 20
    x = _feat(rng, B, C, H, W)
    rois = np.concatenate([_rois("clustered", rng, B, H, W, 8, 24), _rois("borders", rng, B, H, W, 8, 8)])
    want, want_arg = ref.forward(x, rois, 0.125, 7, 7)
    got, got_arg = _gpu_forward(x, rois, 0.125, 7, cuda, True)
    np.testing.assert_array_equal(got_arg, want_arg)
    np.testing.assert_array_equal(got, want)


def test_fp16_boundary_is_exact(cuda):
    rng = np.random.default_rng(5)
    x = _feat(rng, 2, 16, 20, 24).astype(np.float16)
    rois = np.round(_rois("random", rng, 2, 20, 24, 8, 20)).astype(np.float16)   # fp16-representable corners
    want, want_arg = ref.forward(x.astype(np.float32), rois.astype(np.float32), 0.125, 7, 7)
    for nhwc in (True, False):
        xt = torch.from_numpy(x).to(cuda)
        if nhwc:
            xt = xt.contiguous(memory_format=CL)
        out = ROILoopPool((7, 7), 0.125)(xt, torch.from_numpy(rois).to(cuda))
        assert out.dtype == torch.float16
        np.testing.assert_array_equal(out.cpu().numpy(), want.astype(np.float16))


def test_module_surface(cuda):
    m = ROILoopPool((7, 7), 0.125)
    assert repr(m) == "ROILoopPool(output_size=(7, 7), spatial_scale=0.125)"
    x = torch.rand(1, 4, 10, 10, device=cuda)
    out = m(x, torch.tensor([[0, 0, 0, 40, 40.]], device=cuda))
    assert out.shape == (3, 4, 7, 7)


def test_pooler_row_order_single_and_multi_level(cuda):
    rng = np.random.default_rng(9)
    B, C = 2, 8
    feats_np = [_feat(rng, B, C, 64 // s, 64 // s) for s in (4, 8)]
    boxes = [np.abs(_rois("random", rng, 1, 8, 8, 8, n)[:, 1:]) for n in (7, 5)]
    box_lists = [Boxes(torch.from_numpy(b).to(cuda)) for b in boxes]
    feats = [torch.from_numpy(f).to(cuda).contiguous(memory_format=CL) for f in feats_np]
    # one level: the operator's own rows
    p1 = ROIPooler(7, (1.0 / 8,), 0, "ROILoopPool")
    out1 = p1([feats[1]], box_lists).cpu().numpy()
    rois = np.concatenate([np.concatenate([np.full((len(b), 1), i, np.float32), b], 1) for i, b in enumerate(boxes)])
    want1, _ = ref.forward(feats_np[1], rois, 1.0 / 8, 7, 7)
    np.testing.assert_array_equal(out1, want1)
    # two levels: row i of a level goes to rows i, i + N, i + 2N
    p2 = ROIPooler(7, (1.0 / 4, 1.0 / 8), 0, "ROILoopPool", canonical_box_size=16, canonical_level=3)
    level_ids = [torch.from_numpy(np.arange(len(b)) % 2).to(cuda) for b in boxes]
    out2 = p2(feats, box_lists, level_ids=level_ids).cpu().numpy()
    N = len(rois)
    lvl = np.concatenate([np.arange(len(b)) % 2 for b in boxes])
    for level, scale in ((0, 0.25), (1, 0.125)):
        idx = np.nonzero(lvl == level)[0]
        want, _ = ref.forward(feats_np[level], rois[idx], scale, 7, 7)
        for k in range(3):
            np.testing.assert_array_equal(out2[idx + k * N], want[k * len(idx):(k + 1) * len(idx)])


@pytest.mark.parametrize("C,nhwc", [(512, True), (6, True), (4, False)], ids=["c512-nhwc", "c6-nhwc", "c4-nchw"])
def test_backward_matches_restatement_and_is_reproducible(cuda, C, nhwc):
    rng = np.random.default_rng(C)
    B, H, W = 2, 20, 24
    x = _feat(rng, B, C, H, W)
    rois = np.concatenate([_rois("clustered", rng, B, H, W, 8, 20), _rois("borders", rng, B, H, W, 8, 6),
                           _rois("degenerate", rng, B, H, W, 8, 4), _rois("large", rng, B, H, W, 8, 2),
                           _rois("stray", rng, B, H, W, 8, 12)])
    R = len(rois)
    g = rng.standard_normal((3 * R, C, 7, 7)).astype(np.float32)
    _, arg = ref.forward(x, rois, 0.125, 7, 7)
    want = ref.backward(g, rois, arg, B, C, H, W)
    xt = torch.from_numpy(x).to(cuda)
    if nhwc:
        xt = xt.contiguous(memory_format=CL)
    xt.requires_grad_(True)
    rt = torch.from_numpy(rois).to(cuda)
    out = ROILoopPool((7, 7), 0.125)(xt, rt)
    gt = torch.from_numpy(g).to(cuda).contiguous(memory_format=CL if nhwc else torch.contiguous_format)
    out.backward(gt)
    got = xt.grad.cpu().numpy()
    tol = 1e-6 * float(np.abs(want).max())
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=tol)
    # a second call on the same inputs: the same bits
    _, argt = roi_loop_pool_forward(xt.detach(), rt, 0.125, 7, 7)
    again = roi_loop_pool_backward(gt, rt, argt, 0.125, 7, 7, B, C, H, W).cpu().numpy()
    np.testing.assert_array_equal(again, got)
    # the documented order, in float32: rois ascending; per roi the box's bins (block 0, then block 1 of each bin)
    # before the outer box's (block 2); bins ph outer, pw inner
    np.testing.assert_array_equal(argt.cpu().numpy(), arg)

    def in_order(t):
        box = np.stack([_rows(t[:R], R), _rows(t[R:2 * R], R)], axis=2).reshape(R, -1, C)
        return np.concatenate([box, _rows(t[2 * R:], R)], axis=1).reshape(-1, C)

    ordered = _sum_in_order(in_order(arg), in_order(g), np.repeat(rois[:, 0], 3 * 49), B, C, H, W)
    np.testing.assert_array_equal(got, ordered)
    # the rois that name no image removed from rois, argmax and grad: the same bits
    keep = torch.from_numpy((rois[:, 0] >= 0) & (rois[:, 0] < B)).to(cuda)
    assert 0 < int(keep.sum()) < R
    keep3 = keep.repeat(3)
    without = roi_loop_pool_backward(gt[keep3], rt[keep], argt[keep3], 0.125, 7, 7, B, C, H, W, nhwc=nhwc).cpu().numpy()
    np.testing.assert_array_equal(without, got)


def test_backward_without_rois_is_zero(cuda):
    x = torch.rand(2, 8, 6, 6, device=cuda).contiguous(memory_format=CL).requires_grad_(True)
    out = ROILoopPool((7, 7), 0.125)(x, torch.zeros((0, 5), device=cuda))
    assert out.shape == (0, 8, 7, 7)
    out.sum().backward()
    assert x.grad is not None and (x.grad == 0).all()
