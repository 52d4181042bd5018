"""The two mining entry points that were only ever run through the whole model — jtsm_near_targets_f32 and the rectangle
painter jtsm_paint_sem_seg (csrc/mining.hip) — against torch-CPU restatements of their rules, bit for bit.  Both decide
integers, and the inputs are built so that the tie-break rules decide some of them.  With them the rectangle mask
targets, jtsm_rect_mask_targets_f32 (csrc/roi_align.hip), against rasterise-then-ROIAlign of the oracle, bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _iou(q, p):
    """pairwise_iou of target q (4,) with proposals p (n, 4) in float32, one operation at a time."""
    area_q = (q[2] - q[0]) * (q[3] - q[1])
    area_p = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    w = (torch.minimum(q[2], p[:, 2]) - torch.maximum(q[0], p[:, 0])).clamp(min=0)
    h = (torch.minimum(q[3], p[:, 3]) - torch.maximum(q[1], p[:, 1])).clamp(min=0)
    inter = w * h
    return torch.where(inter > 0, inter / (area_q + area_p - inter), torch.zeros_like(inter))


def _grid_boxes(g, n):
    """n boxes on an integer grid, about a quarter of them exact copies of earlier rows."""
    xy = torch.randint(0, 9, (n, 2), generator=g)
    wh = torch.randint(1, 7, (n, 2), generator=g)
    b = torch.cat([xy, xy + wh], dim=1).to(torch.float32)
    for i in range(1, n):
        if int(torch.randint(0, 4, (1,), generator=g)) == 0:
            b[i] = b[int(torch.randint(0, i, (1,), generator=g))]
    return b


def _off_by_one_word(t, device):
    """t on the device at an address that is 4 bytes past a 16-byte boundary: neither entry point asks for more."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def test_near_targets_rank_by_iou_then_row(cuda):
    from jtsm_amd.layers.mining import near_targets

    g = torch.Generator().manual_seed(11)
    bags, top_k, G, bg = [300, 7, 41], 10, 4, 20          # 300 rows: every thread of the 256 takes a second pass
    counts = [4, 3, 0]                                    # the last image has no pseudo box at all
    off = [0]
    for n in bags:
        off.append(off[-1] + n)
    R, B = off[-1], len(bags)
    boxes = torch.cat([_grid_boxes(g, n) for n in bags])
    # ~60 % foreground; the rest background or ignored (-1)
    labels = torch.randint(0, bg, (R,), generator=g, dtype=torch.int32)
    kind = torch.randint(0, 10, (R,), generator=g)
    labels[kind >= 6] = bg
    labels[kind == 9] = -1
    fg = (labels != bg) & (labels >= 0)
    pgt = torch.full((B, G, 4), 1e6)                      # slots past counts[b] hold garbage that must not be read as a box
    for b in range(B):
        for j in range(counts[b]):                        # pseudo boxes are proposals of the image, as mined ones are
            pgt[b, j] = boxes[off[b] + int(torch.randint(0, bags[b], (1,), generator=g))]
    assert int(fg[off[1]:off[2]].sum()) < top_k and int(fg[off[2]:].sum()) > 0

    # ---- restatement
    want_near = torch.full((B, G, top_k), -1, dtype=torch.int32)
    rank_ties = 0
    for b in range(B):
        rows = torch.arange(off[b], off[b + 1])[fg[off[b]:off[b + 1]]]
        for j in range(counts[b]):
            v = _iou(pgt[b, j], boxes[rows])
            sv, order = torch.sort(v, descending=True, stable=True)      # equal IoUs stay in ascending row order
            k = min(top_k, rows.numel())
            want_near[b, j, :k] = rows[order[:k]].to(torch.int32)
            m = min(k, rows.numel() - 1)                                 # neighbours of which at least one is listed
            rank_ties += int((sv[:m] == sv[1:m + 1]).sum())
    want_matched = torch.full((R,), -1, dtype=torch.int32)
    first_max_ties = 0
    for b in range(B):
        cand = want_near[b, :counts[b]].reshape(-1)                      # target-major, rank-minor
        cand = cand[cand >= 0].to(torch.int64)
        if cand.numel() == 0:
            continue
        for r in range(off[b], off[b + 1]):
            if not fg[r]:
                continue
            v = torch.stack([_iou(boxes[c], boxes[r:r + 1])[0] for c in cand])
            at = int((v == v.max()).nonzero()[0])                        # the first maximum
            want_matched[r] = int(cand[at])
            first_max_ties += int(((v == v.max()) & (cand != cand[at])).any())
    assert rank_ties > 0 and first_max_ties > 0, "the inputs hold no tie for the row order to decide"
    assert (want_near[1, :counts[1], -1] == -1).all() and (want_near[2] == -1).all()

    # ---- the kernels, on boxes that are not 16-byte aligned
    dev_pgt = dict(boxes=_off_by_one_word(pgt, cuda))
    near, matched = near_targets(_off_by_one_word(boxes, cuda), torch.tensor(off, dtype=torch.int32, device=cuda),
                                 labels.to(cuda), bg, dev_pgt, torch.tensor(counts, dtype=torch.int32, device=cuda), top_k)
    assert torch.equal(near.cpu(), want_near), (near.cpu() != want_near).nonzero()[:5]
    assert torch.equal(matched.cpu(), want_matched), (matched.cpu() != want_matched).nonzero()[:5]


def test_paint_sem_seg_rectangles_and_missing_rule(cuda):
    from jtsm_amd.layers.mining import paint_sem_seg

    B, H, W, G, base, erode = 3, 37, 53, 8, 10, 2.0       # 1961 pixels: the last block of 256 is partial
    boxes = torch.full((B, G, 4), -7.0)
    classes = torch.full((B, G), 63, dtype=torch.int32)   # slots past counts[b]: garbage that must paint nothing
    scores = torch.full((B, G), 9.0)
    lists = [
        # image 0: slots 2 and 3 score the same (the index ranks them); slot 1 lies entirely under the better slot 0, so
        # its class is painted over and the missing rule paints it once more
        [((2, 2, 44, 32), 11, 0.9), ((10, 8, 30, 24), 12, 0.5), ((28, 10, 52, 36), 13, 0.7), ((24, 14, 50, 34), 14, 0.7),
         ((0, 20, 20, 36), 15, 0.6)],
        # image 1: slot 0 is narrower than 2 * erode (missing, and a repaint paints nothing); class 16 comes twice
        [((5, 5, 8, 30), 15, 0.8), ((10, 4, 30, 20), 16, 0.3), ((20, 10, 45, 33), 16, 0.4), ((12.5, 6.25, 28.5, 18.75), 17, 0.35)],
        [],
    ]
    for b, items in enumerate(lists):
        for j, (bx, c, s) in enumerate(items):
            boxes[b, j] = torch.tensor(bx, dtype=torch.float32)
            classes[b, j] = c
            scores[b, j] = s
    counts = torch.tensor([len(items) for items in lists], dtype=torch.int32)

    # ---- restatement: paint in ascending (score, index) order, then the missing rule in list order
    xs = (torch.arange(W, dtype=torch.float32) + 0.5)[None, :]
    ys = (torch.arange(H, dtype=torch.float32) + 0.5)[:, None]
    e = torch.tensor(erode, dtype=torch.float32)

    def inside(bx):
        return (xs >= bx[0] + e) & (xs <= bx[2] - e) & (ys >= bx[1] + e) & (ys <= bx[3] - e)

    want = torch.zeros((B, H, W), dtype=torch.int64)
    fired = repainted = 0
    for b in range(B):
        n = int(counts[b])
        for j in sorted(range(n), key=lambda j: (float(scores[b, j]), j)):
            want[b][inside(boxes[b, j])] = int(classes[b, j]) - base
        for j in range(n):
            v = int(classes[b, j]) - base
            if int((want[b] == v).sum()) == 0:
                fired += 1
                repainted += int(inside(boxes[b, j]).sum())
                want[b][inside(boxes[b, j])] = v
    assert fired >= 2 and repainted > 0, "the missing-class rule never fired"
    assert not inside(boxes[1, 0]).any() and (want[2] == 0).all()
    tie = inside(boxes[0, 2]) & inside(boxes[0, 3]) & ~inside(boxes[0, 0])
    assert tie.any() and (want[0][tie] == 14 - base).all()    # equal scores: the later slot ends on top

    got = paint_sem_seg(boxes.to(cuda), classes.to(cuda), scores.to(cuda), counts.to(cuda), base, H, W, erode)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want), (got.cpu() != want).nonzero()[:5]


# ---- rect_mask_targets (csrc/roi_align.hip: rect_mask_targets_kernel) ------------------------------------------------------
RECT_H, RECT_W = 300, 340


def _rect_inputs(seed=31):
    """24 rois in a 300 x 340 image with the pseudo-GT rectangle matched to each: mostly the roi moved by a few pixels,
    so that the shrunk rectangle's edge crosses the roi's bins."""
    g = torch.Generator().manual_seed(seed)
    n = 24
    wh = torch.rand(n, 2, generator=g) * 197 + 3                    # sides of 3 to 200 pixels
    xy = torch.rand(n, 2, generator=g) * (torch.tensor([RECT_W, RECT_H]) - wh)
    rois = torch.cat([xy, xy + wh], 1)
    rois[0] = torch.tensor([-40.0, -30.0, 90.5, 120.25])            # partly outside
    rois[1] = torch.tensor([5.0, 6.0, 7.5, 9.0])                    # tiny
    rois[2] = torch.tensor([4.0, 3.0, 336.5, 297.25])               # nearly the whole image
    rects = rois + (torch.rand(n, 4, generator=g) * 12 - 6)
    rects[1] = torch.tensor([1.0, 2.0, 8.5, 9.5])                   # (shrunk by 2, its corner lies inside the tiny roi)
    rects[3] = rois[3]
    rects[3, 2] = rois[3, 0] + 3.0                                  # narrower than 2 * erode
    rects[4] = torch.tensor([300.0, 250.0, 335.0, 295.0])           # disjoint from its roi ...
    rois[4] = torch.tensor([20.0, 30.0, 120.0, 90.0])               # ... which is this
    rects[5] = torch.tensor([0.0, 0.0, float(RECT_W), float(RECT_H)])   # the whole image
    return rois, rects


def _rect_reference(rois, rects, side, erode):
    """The rectangle rasterised (oracle/model.py: eroded_rect_masks) and cropped by the C restatement of ROIAlign, as
    BitMasks.crop_and_resize does it: scale 1, adaptive sampling, aligned, >= 0.5."""
    from oracle import model as OM
    from oracle import pooling as P

    masks = OM.eroded_rect_masks(rects, RECT_H, RECT_W, erode)
    rr = torch.cat([torch.arange(rois.shape[0], dtype=torch.float32)[:, None], rois], 1)
    return torch.from_numpy(P.roi_align_forward(masks[:, None].numpy(), rr.numpy(), 1.0, side, side, 0, True))[:, 0] >= 0.5


@pytest.mark.parametrize("side,erode", [(28, 2.0), (28, 0.0), (7, 2.0)], ids=["28-erode2", "28-erode0", "7-erode2"])
def test_rect_mask_targets_bit_exact_vs_rasterise_then_roi_align(cuda, side, erode):
    """The kernel evaluates the shrunk rectangle analytically at every ROIAlign tap (nothing is rasterised); the oracle
    rasterises it and crops.  Bits must agree exactly, as for its siblings paste_crop_targets and sp_mask_targets
    (test_hip_losses.py)."""
    from jtsm_amd.layers.mining import rect_mask_targets

    rois, rects = _rect_inputs()
    want = _rect_reference(rois, rects, side, erode)
    if erode > 0:
        assert not want[3].any()                                    # narrower than 2 * erode: an empty mask
    assert not want[4].any() and want[5].all()                      # disjoint; the whole image (eroded: less than a bin)
    if (side, erode) == (28, 2.0):
        assert 0.1 < float(want.float().mean()) < 0.9
    got = rect_mask_targets(rois.to(cuda), rects.to(cuda), side, RECT_H, RECT_W, erode).cpu()
    assert got.shape == want.shape and got.dtype == torch.bool
    assert torch.equal(got, want), (got != want).nonzero()[:5]


def test_rect_mask_targets_of_no_roi(cuda):
    from jtsm_amd.layers.mining import rect_mask_targets

    got = rect_mask_targets(torch.zeros(0, 4, device=cuda), torch.zeros(0, 4, device=cuda), 28, RECT_H, RECT_W)
    assert got.shape == (0, 28, 28) and got.dtype == torch.bool
