"""PointRend operators (jtsm_amd/csrc/point_rend.hip) behind ctypes, and their autograd functions.

point_gather / point_sample / point_sample_fine_grained_features
                       <- point_sample, point_sample_fine_grained_features   (projects/PointRend/point_rend/point_features.py:28-51, 155-225)
point_select / get_uncertain_point_coords_with_randomness
                       <- get_uncertain_point_coords_with_randomness + calculate_uncertainty
                                                                             (point_features.py:72-125, mask_head.py:23-45)
point_loss / roi_mask_point_loss
                       <- roi_mask_point_loss                                (point_head.py:22-96)
point_subdivide, point_scatter, get_uncertain_point_coords_on_grid
                       <- the loop body of _forward_mask_point               (mask_head.py:245-275, point_features.py:128-152)

The fused path: `point_gather` writes the features of every source — FPN levels shared by an image's rois
and per-roi coarse logits — side by side into one (R * P, row_stride) row buffer, points-major and channels-minor,
which is the 1x1-contraction operand of the point MLP.  The functions with the reference's names wrap it and return
the reference's (R, C, P) shapes as views."""
import ctypes as C

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib as L
from . import grad_fan

SHARED, PER_ROI = 0, 1


def _f32(t):
    return t.to(torch.float32).contiguous()


def _geom(t, col, kind):
    """One source, a logical (N, C, H, W) tensor of any strides -> its nine-int64 row of the kernels' table."""
    if t.dim() != 4 or t.dtype != torch.float32:
        raise RuntimeError("point_gather: a source must be float32 (N, C, H, W), got %s %s" % (tuple(t.shape), t.dtype))
    n, c, h, w = t.shape
    sn, sc, sy, sx = t.stride()
    return [h, w, c, col, kind, sn, sc, sy, sx]


def roi_image_index(counts, device):
    """Host counts of rois per image -> int32 (R,) image index of each roi, built on the device."""
    counts = torch.tensor([int(c) for c in counts], dtype=torch.int64)
    return torch.repeat_interleave(torch.arange(len(counts), dtype=torch.int32), counts).to(device, non_blocking=True)


class _PointGather(Function):
    @staticmethod
    def forward(ctx, cfg, boxes, roi_image, points, out, *maps):
        kinds, scales, cols, R, P, side, s2d, row_stride, want_coords = cfg
        L.require_gpu(boxes, roi_image, points, out, *maps)
        if len(maps) != len(kinds) or not 1 <= len(maps) <= 8:
            raise RuntimeError("point_gather: %d sources for %d kinds (1..8)" % (len(maps), len(kinds)))
        dev = maps[0].device
        ctx.recs = [grad_fan.claim(m) if k == SHARED else None for m, k in zip(maps, kinds)]
        maps = [m.detach() for m in maps]
        geom = []
        for m, k, c in zip(maps, kinds, cols):
            geom += _geom(m, c, k)
            if k == PER_ROI and m.shape[0] != R:
                raise RuntimeError("point_gather: a per-roi source of %d maps for %d rois" % (m.shape[0], R))
        if side == 0:
            if points is None or tuple(points.shape) != (R, P, 2):
                raise RuntimeError("point_gather: points %s for R = %d, P = %d" % (
                    None if points is None else tuple(points.shape), R, P))
            points = _f32(points.detach())
        else:
            points = None
        if boxes is not None:
            if tuple(boxes.shape) != (R, 4) or roi_image is None or roi_image.numel() != R:
                raise RuntimeError("point_gather: boxes %s / roi_image for %d rois" % (tuple(boxes.shape), R))
            boxes, roi_image = _f32(boxes.detach()), roi_image.to(torch.int32).contiguous()
        elif SHARED in kinds:
            raise RuntimeError("point_gather: a shared source needs boxes and roi_image")
        if out is None:
            out = torch.empty((R * P, row_stride), dtype=torch.float32, device=dev)
        else:
            if out.dtype != torch.float32 or tuple(out.shape) != (R * P, row_stride) or not out.is_contiguous():
                raise RuntimeError("point_gather: out must be contiguous float32 (%d, %d)" % (R * P, row_stride))
            ctx.mark_dirty(out)
        coords = torch.empty((R, P, 2), dtype=torch.float32, device=dev) if want_coords and boxes is not None else None
        ptrs = (C.c_void_p * len(maps))(*[m.data_ptr() for m in maps])
        g = (C.c_int64 * len(geom))(*geom)
        sc = (C.c_float * len(maps))(*[float(s) for s in scales])
        n_img = min([int(m.shape[0]) for m, k in zip(maps, kinds) if k == SHARED] or [0])
        L.check(L.lib().jtsm_point_gather_forward_f32(ptrs, g, sc, len(maps), n_img, L.ptr(boxes), L.ptr(roi_image),
                                                      L.ptr(points), R, P, side, int(s2d), L.ptr(out), row_stride,
                                                      L.ptr(coords), L.stream()), "point_gather_forward")
        ctx.cfg = cfg
        ctx.shapes = [(tuple(m.shape), tuple(m.stride())) for m in maps]
        ctx.save_for_backward(boxes, roi_image, points)
        if coords is None:
            coords = out.new_zeros(0)
        ctx.mark_non_differentiable(coords)
        return out, coords

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gc):
        kinds, scales, cols, R, P, side, s2d, row_stride, _ = ctx.cfg
        boxes, roi_image, points = ctx.saved_tensors
        g = _f32(g)
        lib = L.lib()
        grads = []
        for i, ((shape, strides), k) in enumerate(zip(ctx.shapes, kinds)):
            if not ctx.needs_input_grad[5 + i]:
                grads.append(None)
                continue
            n, c, h, w = shape
            if k == PER_ROI:
                if any(t == 0 and s > 1 for s, t in zip(shape, strides)):      # an expanded map: a dense gradient
                    d = torch.empty(shape, dtype=torch.float32, device=g.device)
                else:
                    d = torch.empty_strided(shape, strides, dtype=torch.float32, device=g.device)
                sn, sc, sy, sx = d.stride()
                L.check(lib.jtsm_point_gather_backward_roi_f32(L.ptr(g), row_stride, cols[i], L.ptr(points), R, P, side,
                                                               int(s2d), c, h, w, L.ptr(d), sn, sc, sy, sx,
                                                               L.stream()), "point_gather_backward_roi")
                grads.append(d)
                continue
            rec = ctx.recs[i]
            tgt = grad_fan.target(rec, shape, g.device)
            acc = tgt is not None
            d = tgt if acc else torch.empty(shape, dtype=torch.float32, device=g.device,
                                            memory_format=torch.channels_last)
            nbytes = lib.jtsm_point_gather_backward_map_workspace_bytes(R, P, n, h, w)
            ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=g.device)
            L.check(lib.jtsm_point_gather_backward_map_f32(L.ptr(g), row_stride, cols[i], L.ptr(boxes), L.ptr(roi_image),
                                                           L.ptr(points), R, P, side, int(s2d), n, h, w, c,
                                                           float(scales[i]), L.ptr(d), int(acc), L.ptr(ws), ws.numel(),
                                                           L.stream()), "point_gather_backward_map")
            grads.append(None if acc or grad_fan.offer(rec, d) else d)
        return (None, None, None, None, None) + tuple(grads)


def point_gather(sources, boxes=None, roi_image=None, points=None, num_rois=None, grid_side=0, space_to_depth=False,
                 row_stride=None, out=None, want_coords=True):
    """sources: list of (map, kind, scale, first column); map is a logical (N, C, H, W) float32 tensor of any strides
    (channels-last FPN levels and plain coarse logits alike), kind SHARED (indexed by roi_image, read at the image-space
    point) or PER_ROI (one map per roi, read at the box-normalised point; scale ignored).  points (R, P, 2)
    box-normalised, or grid_side > 0 for the regular grid (optionally in space-to-depth row order).
    -> rows (R * P, row_stride) with every source's channels at its columns (other columns keep what `out` held),
    coords_wrt_image (R, P, 2).  One launch; gradients flow to the maps, not to the coordinates."""
    maps = [s[0] for s in sources]
    kinds, scales, cols = tuple(int(s[1]) for s in sources), tuple(float(s[2]) for s in sources), tuple(int(s[3]) for s in sources)
    if grid_side:
        P = int(grid_side) ** 2
        R = int(num_rois if num_rois is not None else boxes.shape[0])
    else:
        R, P = int(points.shape[0]), int(points.shape[1])
    width = max(c + m.shape[1] for c, m in zip(cols, maps))
    row_stride = int(row_stride if row_stride is not None else (out.shape[1] if out is not None else width))
    if row_stride < width:
        raise RuntimeError("point_gather: rows of %d floats for columns up to %d" % (row_stride, width))
    cfg = (kinds, scales, cols, R, P, int(grid_side), bool(space_to_depth), row_stride, bool(want_coords))
    rows, coords = _PointGather.apply(cfg, boxes, roi_image, points, out, *maps)
    return rows, (coords if coords.numel() else None)


# ---- the reference's names ---------------------------------------------------------------------------------------------
def point_sample(input, point_coords, **kwargs):
    """input (N, C, H, W) — channels-last in memory here, any strides are read in place — and point_coords (N, P, 2) or
    (N, Hgrid, Wgrid, 2) in [0, 1] x [0, 1] -> (N, C, P) or (N, C, Hgrid, Wgrid), a view of the points-major rows.
    Only grid_sample's bilinear / zeros / align_corners=False form exists."""
    if kwargs.get("align_corners", False) or kwargs.get("mode", "bilinear") != "bilinear" or \
            kwargs.get("padding_mode", "zeros") != "zeros":
        raise NotImplementedError("point_sample: only mode='bilinear', padding_mode='zeros', align_corners=False")
    grid = point_coords.dim() == 4
    pts = point_coords.reshape(point_coords.shape[0], -1, 2) if grid else point_coords
    n, c, p = input.shape[0], input.shape[1], pts.shape[1]
    if n == 0 or p == 0:
        out = input.new_zeros((n, c, p)) + input.sum() * 0
    else:
        rows, _ = point_gather([(input, PER_ROI, 1.0, 0)], points=pts, want_coords=False)
        out = rows.view(n, p, c).permute(0, 2, 1)
    return out.reshape(n, c, point_coords.shape[1], point_coords.shape[2]) if grid else out


def generate_regular_grid_point_coords(R, side_size, device):
    """(R, side_size^2, 2) cell centres of the regular grid, row-major, in the kernels' fp32 expression
    ((2 i + 1) / side - 1) * 0.5 + 0.5 (side_size values formed on the host, where every step is rounded as the
    kernels round it; the heads use point_gather's grid mode and never build this tensor)."""
    c = ((2 * torch.arange(side_size, dtype=torch.float32) + 1) / float(side_size) - 1.0) * 0.5 + 0.5
    y, x = torch.meshgrid(c, c, indexing="ij")
    return torch.stack([x, y], dim=-1).view(1, -1, 2).to(device).expand(R, -1, -1)


class UncertaintyOfClasses(object):
    """`lambda logits: calculate_uncertainty(logits, classes)` as an object the selection kernel can look into."""

    def __init__(self, classes):
        self.classes = classes

    def __call__(self, logits):
        return calculate_uncertainty(logits, self.classes)


def calculate_uncertainty(logits, classes):
    """(R, C, ...) or (R, 1, ...) logits -> (R, 1, ...) = -|logit of the roi's class| (mask_head.py:23-45)."""
    if logits.shape[1] == 1:
        picked = logits.clone()
    else:
        picked = logits[torch.arange(logits.shape[0], device=logits.device), classes].unsqueeze(1)
    return -(torch.abs(picked))


@torch.no_grad()
def point_select(coarse_logits, classes, candidates, randoms, num_points, return_chosen=False):
    """coarse_logits (R, C, S, S); classes (R) or None for C == 1; candidates (R, K, 2), randoms (R, P - U, 2) uniform
    draws -> (R, P, 2): the U = K-candidates' most uncertain first (ties to the lower candidate), then the randoms."""
    L.require_gpu(coarse_logits, classes, candidates, randoms)
    r, c, s, s2 = coarse_logits.shape
    k = int(candidates.shape[1])
    p = int(num_points)
    u = p - (int(randoms.shape[1]) if randoms is not None else 0)
    if s != s2 or (c > 1 and (classes is None or classes.numel() != r)) or tuple(candidates.shape) != (r, k, 2) or \
            (randoms is not None and tuple(randoms.shape) != (r, p - u, 2)):
        raise RuntimeError("point_select: logits %s / candidates %s / randoms %s" % (
            tuple(coarse_logits.shape), tuple(candidates.shape), None if randoms is None else tuple(randoms.shape)))
    logits = coarse_logits.detach().to(torch.float32).contiguous()
    classes = None if c == 1 else classes.to(torch.int64).contiguous()
    candidates = _f32(candidates)
    randoms = None if randoms is None or u == p else _f32(randoms)
    out = torch.empty((r, p, 2), dtype=torch.float32, device=logits.device)
    chosen = torch.empty((r, u), dtype=torch.int32, device=logits.device) if return_chosen else None
    L.check(L.lib().jtsm_point_select_f32(L.ptr(logits), r, c, s, L.ptr(classes), L.ptr(candidates), k, L.ptr(randoms),
                                          u, p, L.ptr(out), L.ptr(chosen), L.stream()), "point_select")
    return (out, chosen) if return_chosen else out


@torch.no_grad()
def get_uncertain_point_coords_with_randomness(coarse_logits, uncertainty_func, num_points, oversample_ratio,
                                               importance_sample_ratio):
    """The reference's signature.  `uncertainty_func` is an UncertaintyOfClasses (or the class tensor itself, or None
    for class-agnostic logits): the kernel forms -|logit| of that class itself, and no other function can be passed to
    it.  torch.rand is called with the reference's shapes in the reference's order, so a seeded run draws its numbers."""
    assert oversample_ratio >= 1
    assert 0 <= importance_sample_ratio <= 1
    if isinstance(uncertainty_func, UncertaintyOfClasses):
        classes = uncertainty_func.classes
    elif uncertainty_func is None or isinstance(uncertainty_func, torch.Tensor):
        classes = uncertainty_func
    else:
        raise NotImplementedError("get_uncertain_point_coords_with_randomness: the uncertainty is -|logit| of a class; "
                                  "pass UncertaintyOfClasses(classes)")
    r = coarse_logits.shape[0]
    num_sampled = int(num_points * oversample_ratio)
    num_uncertain = int(importance_sample_ratio * num_points)
    num_random = num_points - num_uncertain
    candidates = torch.rand(r, num_sampled, 2, device=coarse_logits.device)
    randoms = torch.rand(r, num_random, 2, device=coarse_logits.device) if num_random > 0 else None
    if r == 0:
        return coarse_logits.new_zeros((0, num_points, 2))
    return point_select(coarse_logits, classes, candidates, randoms, num_points)


def point_sample_fine_grained_features(features_list, feature_scales, boxes, point_coords):
    """features_list: (N, C_l, H_l, W_l) maps; boxes: list of N Boxes (or (R_i, 4) tensors); point_coords (R, P, 2)
    -> (R, sum C_l, P) as a view of the row buffer, and point_coords_wrt_image (R, P, 2).  One launch."""
    tensors = [b.tensor if hasattr(b, "tensor") else b for b in boxes]
    cat = torch.cat(tensors) if len(tensors) != 1 else tensors[0]
    r, p = int(point_coords.shape[0]), int(point_coords.shape[1])
    ctot = sum(int(f.shape[1]) for f in features_list)
    if r == 0:
        zero = sum(f.sum() for f in features_list) * 0
        return point_coords.new_zeros((0, ctot, p)) + zero, point_coords.new_zeros((0, p, 2))
    roi_image = roi_image_index([t.shape[0] for t in tensors], cat.device)
    sources, col = [], 0
    for f, s in zip(features_list, feature_scales):
        sources.append((f, SHARED, s, col))
        col += int(f.shape[1])
    rows, coords = point_gather(sources, cat, roi_image, point_coords)
    return rows.view(r, p, ctot).permute(0, 2, 1), coords


@torch.no_grad()
def get_point_coords_wrt_image(boxes_coords, point_coords):
    """p * (x2 - x1) + x1 (point_features.py:201-225).  A helper for callers outside the heads, which get these
    coordinates from point_gather; written with tensor ops on (R, P, 2) floats."""
    out = point_coords.clone()
    out[:, :, 0] = out[:, :, 0] * (boxes_coords[:, None, 2] - boxes_coords[:, None, 0])
    out[:, :, 1] = out[:, :, 1] * (boxes_coords[:, None, 3] - boxes_coords[:, None, 1])
    out[:, :, 0] += boxes_coords[:, None, 0]
    out[:, :, 1] += boxes_coords[:, None, 1]
    return out


class _PointLoss(Function):
    @staticmethod
    def forward(ctx, logits, classes, masks, roi_image, matched, coords, P):
        L.require_gpu(logits, classes, roi_image, matched, coords, *masks)
        rows, c = int(logits.shape[0]), int(logits.shape[1])
        if logits.dim() != 2 or logits.dtype != torch.float32 or rows % P:
            raise RuntimeError("point_loss: logits %s %s for P = %d" % (tuple(logits.shape), logits.dtype, P))
        r = rows // P
        if logits.stride(1) != 1 and c > 1 or (rows > 1 and logits.stride(0) < c):
            logits = logits.contiguous()
        ld = logits.stride(0) if rows > 1 else c
        dev = logits.device
        if len(masks) > 64:
            raise RuntimeError("point_loss: %d images (at most 64 per call)" % len(masks))
        keep, geom = [], []
        for m in masks:
            if m is None or m.shape[0] == 0:
                keep.append(None)
                geom += [1, 1, 0]
                continue
            if m.dim() != 3 or m.dtype not in (torch.uint8, torch.bool):
                raise RuntimeError("point_loss: bitmasks must be (G, H, W) uint8 / bool, got %s %s" % (tuple(m.shape), m.dtype))
            m = m.contiguous()
            keep.append(m)
            geom += [int(m.shape[1]), int(m.shape[2]), int(m.shape[0])]
        classes = None if c == 1 else classes.to(torch.int64).contiguous()
        if rows and (roi_image.numel() != r or matched.numel() != r or tuple(coords.shape) != (r, P, 2) or
                     (c > 1 and classes.numel() != r)):
            raise RuntimeError("point_loss: %d rois but roi_image %d / matched %d / coords %s" % (
                r, roi_image.numel(), matched.numel(), tuple(coords.shape)))
        roi_image, matched = roi_image.to(torch.int32).contiguous(), matched.to(torch.int32).contiguous()
        coords = _f32(coords)
        lib = L.lib()
        loss = torch.empty((), dtype=torch.float32, device=dev)
        stats = torch.empty(2, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.jtsm_point_loss_workspace_bytes(r, P), dtype=torch.uint8, device=dev)
        ptrs = (C.c_void_p * max(len(keep), 1))(*[None if m is None else m.data_ptr() for m in keep])
        g = (C.c_int32 * max(len(geom), 1))(*geom)
        L.check(lib.jtsm_point_loss_forward_f32(L.ptr(logits), ld, r, P, c, L.ptr(classes), ptrs, g, len(keep),
                                                L.ptr(roi_image), L.ptr(matched), L.ptr(coords), L.ptr(loss),
                                                L.ptr(stats), L.ptr(ws), L.stream()), "point_loss_forward")
        ctx.save_for_backward(logits, classes, ws)
        ctx.cfg = (r, P, c, ld)
        targets = ws[:4 * rows].view(torch.float32)
        ctx.mark_non_differentiable(stats, targets)
        return loss, stats, targets

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gs, _gt):
        logits, classes, ws = ctx.saved_tensors
        r, P, c, ld = ctx.cfg
        d = torch.empty((r * P, c), dtype=torch.float32, device=logits.device)
        g = _f32(g)
        L.check(L.lib().jtsm_point_loss_backward_f32(L.ptr(logits), ld, r, P, c, L.ptr(classes), L.ptr(g), L.ptr(ws),
                                                     L.ptr(d), c, L.stream()), "point_loss_backward")
        return d, None, None, None, None, None, None


def point_loss(logits_rows, classes, masks, roi_image, matched, coords_wrt_image, num_points, return_details=False):
    """logits_rows (R * P, C) points-major; classes (R) int64 (None for C == 1); masks: per image a (G, H, W) uint8 /
    bool tensor (None or empty: no instance); roi_image, matched (R): the roi's image and its instance there;
    coords_wrt_image (R, P, 2).  -> the mean BCE-with-logits against the bilinearly sampled bitmask; with
    return_details also stats (int32 [accurate rows, rows], as point_rend/accuracy counts them) and the soft targets
    (R * P).  R == 0 gives 0 with a zero gradient."""
    loss, stats, targets = _PointLoss.apply(logits_rows, classes, list(masks), roi_image, matched, coords_wrt_image,
                                            int(num_points))
    return (loss, stats, targets) if return_details else loss


def roi_mask_point_loss(mask_logits, instances, points_coord):
    """The reference's signature: mask_logits (R, C, P) or (R, 1, P); instances with `gt_masks` (the rois' own
    (R_i, H, W) bitmasks, a tensor or an object with `.tensor`) and `gt_classes`; points_coord (R, P, 2) in image
    space.  The heads call point_loss on the row buffer instead and skip the transposition made here."""
    r, c, p = mask_logits.shape
    masks, classes, counts = [], [], []
    for inst in instances:
        if len(inst) == 0:
            continue
        m = inst.gt_masks
        m = m.tensor if hasattr(m, "tensor") else m
        if not isinstance(m, torch.Tensor) or m.dim() != 3:
            raise TypeError("Point head works with GT in 'bitmask' format. Set INPUT.MASK_FORMAT to 'bitmask'.")
        masks.append(m)
        counts.append(int(m.shape[0]))
        classes.append(inst.gt_classes.to(torch.int64))
    if not masks:
        return mask_logits.sum() * 0
    dev = mask_logits.device
    roi_image = roi_image_index(counts, dev)
    matched = torch.cat([torch.arange(n, dtype=torch.int32) for n in counts]).to(dev, non_blocking=True)
    rows = mask_logits.permute(0, 2, 1).reshape(r * p, c)
    return point_loss(rows, None if c == 1 else torch.cat(classes), masks, roi_image, matched, points_coord, p)


@torch.no_grad()
def point_subdivide(mask_logits, num_points):
    """One subdivision step on one channel: (R, 1, H, W) -> the x2 bilinear map (R, 1, 2H, 2W) and, when num_points > 0,
    the min(4HW, num_points) most uncertain cells: indices (R, n) int64 and cell-centre coords (R, n, 2), most
    uncertain first, ties to the lower index.  num_points == 0 only up-samples (the reference's skip rule)."""
    L.require_gpu(mask_logits)
    r, c, h, w = mask_logits.shape
    if c != 1:
        raise RuntimeError("point_subdivide: one channel per roi (the predicted class's), got %s" % (tuple(mask_logits.shape),))
    x = _f32(mask_logits)
    n = min(4 * h * w, int(num_points))
    out = torch.empty((r, 1, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
    idx = torch.empty((r, n), dtype=torch.int64, device=x.device) if n else None
    coords = torch.empty((r, n, 2), dtype=torch.float32, device=x.device) if n else None
    L.check(L.lib().jtsm_point_subdivide_f32(L.ptr(x), r, h, w, L.ptr(out), n, L.ptr(idx), L.ptr(coords), L.stream()),
            "point_subdivide")
    return out, idx, coords


@torch.no_grad()
def get_uncertain_point_coords_on_grid(uncertainty_map, num_points):
    """The reference's signature on a given (R, 1, H, W) uncertainty map: indices (R, n) and coords (R, n, 2) of the
    n = min(H W, num_points) largest values, in (value descending, index ascending) order."""
    L.require_gpu(uncertainty_map)
    r, c, h, w = uncertainty_map.shape
    if c != 1:
        raise RuntimeError("get_uncertain_point_coords_on_grid: (R, 1, H, W), got %s" % (tuple(uncertainty_map.shape),))
    x = _f32(uncertainty_map)
    n = min(h * w, int(num_points))
    idx = torch.empty((r, n), dtype=torch.int64, device=x.device)
    coords = torch.empty((r, n, 2), dtype=torch.float32, device=x.device)
    if n:
        L.check(L.lib().jtsm_point_topk_grid_f32(L.ptr(x), r, h, w, n, L.ptr(idx), L.ptr(coords), L.stream()),
                "point_topk_grid")
    return idx, coords


@torch.no_grad()
def point_scatter(mask_logits, indices, point_logits_rows, classes):
    """mask_logits (R, 1, H, W) contiguous, changed in place: cell indices[r, j] <- point_logits_rows[r * n + j,
    classes[r]] (column 0 when the rows have one column)."""
    L.require_gpu(mask_logits, indices, point_logits_rows, classes)
    r, c1, h, w = mask_logits.shape
    n, c = int(indices.shape[1]), int(point_logits_rows.shape[1])
    if c1 != 1 or not mask_logits.is_contiguous() or mask_logits.dtype != torch.float32 or \
            point_logits_rows.shape[0] != r * n or point_logits_rows.dtype != torch.float32:
        raise RuntimeError("point_scatter: map %s / indices %s / rows %s" % (
            tuple(mask_logits.shape), tuple(indices.shape), tuple(point_logits_rows.shape)))
    rows = point_logits_rows if point_logits_rows.stride(1) == 1 or c == 1 else point_logits_rows.contiguous()
    ld = rows.stride(0) if rows.shape[0] > 1 else c
    if ld < c:
        rows, ld = rows.contiguous(), c
    classes = None if c == 1 else classes.to(torch.int64).contiguous()
    indices = indices.to(torch.int64).contiguous()
    L.check(L.lib().jtsm_point_scatter_f32(L.ptr(rows), ld, r, n, c, L.ptr(classes), L.ptr(indices), h * w,
                                           L.ptr(mask_logits), L.stream()), "point_scatter")
    return mask_logits
