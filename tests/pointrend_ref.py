"""Host restatement of the PointRend operators (jtsm_amd/csrc/point_rend.hip), written from the definitions:
grid_sample(bilinear, zeros, align_corners=False), point_features.py's coordinate conventions, BCE-with-logits and
F.interpolate(scale_factor=2, bilinear).  NumPy; every function takes the dtype it computes in — float64 is the
yardstick for the float quantities, float32 (each operation rounded, the kernels' order) decides what a float64 value
cannot: which side of 1.0 a soft target falls on.  Also the inputs of the recorded cases, regenerated from seeds
(tests/golden/make_pointrend_golden.py stores seeds and results only)."""
import numpy as np
import torch

F32, F64 = np.float32, np.float64


# ---- bilinear sampling ------------------------------------------------------------------------------------------------
def taps(px, py, W, H, dt):
    """Normalised points -> north-west cell (as floats) and the weights nw, ne, sw, se."""
    px, py = np.asarray(px, dt), np.asarray(py, dt)
    one, two = dt(1), dt(2)
    ix = (((two * px - one) + one) * dt(W) - one) / two
    iy = (((two * py - one) + one) * dt(H) - one) / two
    x0, y0 = np.floor(ix), np.floor(iy)
    x1, y1 = x0 + one, y0 + one
    w = [(x1 - ix) * (y1 - iy), (ix - x0) * (y1 - iy), (x1 - ix) * (iy - y0), (ix - x0) * (iy - y0)]
    return x0, y0, w


def sample(m, px, py, dt):
    """m (C, H, W); px, py (P,) normalised -> (P, C), taps added nw, ne, sw, se, zero outside."""
    C, H, W = m.shape
    x0, y0, w = taps(px, py, W, H, dt)
    out = np.zeros((len(x0), C), dt)
    for k in range(4):
        x, y = x0 + (k & 1), y0 + (k >> 1)
        ok = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
        xi, yi = np.where(ok, x, 0).astype(np.int64), np.where(ok, y, 0).astype(np.int64)
        v = m[:, yi, xi].T.astype(dt)
        out = out + np.where(ok[:, None], v * w[k][:, None], dt(0))
    return out


def sample_adjoint(g, px, py, shape, dt=F64):
    """g (P, C) -> gradient (C, H, W) of sample()."""
    C, H, W = shape
    x0, y0, w = taps(px, py, W, H, dt)
    d = np.zeros((C, H, W), dt)
    for k in range(4):
        x, y = x0 + (k & 1), y0 + (k >> 1)
        ok = (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
        for p in np.nonzero(ok)[0]:
            d[:, int(y[p]), int(x[p])] += g[p].astype(dt) * w[k][p]
    return d


def grid_points(side, s2d=False, dt=F64):
    """(side^2, 2) cell centres of the regular grid; row-major, or in space-to-depth order."""
    c = ((dt(2) * np.arange(side).astype(dt) + dt(1)) / dt(side) - dt(1)) * dt(0.5) + dt(0.5)
    if s2d:
        hb = side // 2
        q = np.arange(side * side)
        blk = q >> 2
        y, x = 2 * (blk // hb) + ((q >> 1) & 1), 2 * (blk % hb) + (q & 1)
    else:
        y, x = np.divmod(np.arange(side * side), side)
    return np.stack([c[x], c[y]], -1)


def coords_wrt_image(boxes, points, dt):
    b, p = boxes.astype(dt), points.astype(dt)
    x = p[..., 0] * (b[:, None, 2] - b[:, None, 0]) + b[:, None, 0]
    y = p[..., 1] * (b[:, None, 3] - b[:, None, 1]) + b[:, None, 1]
    return np.stack([x, y], -1)


def gather(fine, scales, coarse, boxes, roi_image, points, dt=F64):
    """fine: list of (N, C, H, W); coarse (R, Cc, S, S) or None -> rows (R * P, sum C + Cc), coords (R, P, 2)."""
    R, P = points.shape[:2]
    pim = coords_wrt_image(boxes, points, dt)
    cols = []
    for f, s in zip(fine, scales):
        H, W = f.shape[2:]
        sx, sy = dt(W) / dt(s), dt(H) / dt(s)
        cols.append(np.concatenate([sample(f[roi_image[r]], pim[r, :, 0] / sx, pim[r, :, 1] / sy, dt)
                                    for r in range(R)]) if R else np.zeros((0, f.shape[1]), dt))
    if coarse is not None:
        cols.append(np.concatenate([sample(coarse[r], points[r, :, 0], points[r, :, 1], dt) for r in range(R)])
                    if R else np.zeros((0, coarse.shape[1]), dt))
    return np.concatenate(cols, 1), pim


def gather_adjoint(g, fine_shapes, scales, coarse_shape, boxes, roi_image, points):
    """g (R * P, Ctot) -> gradients of the fine maps and of the coarse logits (float64)."""
    R, P = points.shape[:2]
    pim = coords_wrt_image(boxes, points, F64)
    out, col = [], 0
    for shape, s in zip(fine_shapes, scales):
        N, C, H, W = shape
        d = np.zeros(shape, F64)
        for r in range(R):
            d[roi_image[r]] += sample_adjoint(g[r * P:(r + 1) * P, col:col + C], pim[r, :, 0] / (W / s),
                                              pim[r, :, 1] / (H / s), (C, H, W))
        out.append(d)
        col += C
    dc = None
    if coarse_shape is not None:
        C = coarse_shape[1]
        dc = np.stack([sample_adjoint(g[r * P:(r + 1) * P, col:col + C], points[r, :, 0], points[r, :, 1],
                                      coarse_shape[1:]) for r in range(R)]) if R else np.zeros(coarse_shape, F64)
    return out, dc


# ---- selection --------------------------------------------------------------------------------------------------------
def order(u):
    """Indices in (value descending, index ascending) order: our tie rule."""
    return np.lexsort((np.arange(len(u)), -u))


def uncertainties(coarse, classes, cand, dt=F64):
    """coarse (R, C, S, S), cand (R, K, 2) -> (R, K) = -|sampled logit of the roi's class| (channel 0 when C == 1)."""
    R, C = coarse.shape[:2]
    ch = np.zeros(R, np.int64) if C == 1 else classes
    return np.stack([-np.abs(sample(coarse[r, ch[r]:ch[r] + 1], cand[r, :, 0], cand[r, :, 1], dt)[:, 0])
                     for r in range(R)]) if R else np.zeros((0, cand.shape[1]), dt)


def select(coarse, classes, cand, rand, num_uncertain, dt=F64):
    """-> point coords (R, P, 2), chosen candidate indices (R, U) in order, uncertainties (R, K)."""
    u = uncertainties(coarse, classes, cand, dt)
    chosen = np.stack([order(row)[:num_uncertain] for row in u]) if len(u) else np.zeros((0, num_uncertain), np.int64)
    pts = np.stack([cand[r, chosen[r]] for r in range(len(u))]) if len(u) else cand[:, :0]
    if rand is not None and rand.shape[1]:
        pts = np.concatenate([pts, rand], 1)
    return pts, chosen, u


def ambiguous(u, num_chosen, margin):
    """Rois whose last chosen and first rejected value (float64) lie within `margin` of each other."""
    out = np.zeros(len(u), bool)
    for r, row in enumerate(u):
        s = np.sort(row)[::-1]
        if 0 < num_chosen < len(s):
            out[r] = s[num_chosen - 1] - s[num_chosen] <= margin
    return out


# ---- loss -------------------------------------------------------------------------------------------------------------
def soft_targets(masks, roi_image, matched, coords, dt=F64):
    """masks: per image (G, h, w) uint8 or None; coords (R, P, 2) image space -> (R, P)."""
    R, P = coords.shape[:2]
    out = np.zeros((R, P), dt)
    for r in range(R):
        m = masks[roi_image[r]]
        if m is None or len(m) == 0:
            continue
        h, w = m.shape[1:]
        c = coords[r].astype(dt)
        out[r] = sample(m[matched[r]][None].astype(dt), c[:, 0] / dt(w), c[:, 1] / dt(h), dt)[:, 0]
    return out


def point_loss(logits, classes, masks, roi_image, matched, coords, P):
    """logits (R * P, C) -> loss, gradient (R * P, C) (float64), soft targets float64 (R * P), and the accuracy count
    with the targets formed in float32 as the kernel forms them."""
    rows, C = logits.shape
    R = rows // P
    if rows == 0:
        return 0.0, np.zeros((0, C), F64), np.zeros(0, F64), 0
    ch = np.zeros(R, np.int64) if C == 1 else classes
    col = np.repeat(ch, P)
    x = logits[np.arange(rows), col].astype(F64)
    t = soft_targets(masks, roi_image, matched, coords, F64).reshape(-1)
    loss = ((1 - t) * x + np.maximum(-x, 0) + np.log1p(np.exp(-np.abs(x)))).mean()
    grad = np.zeros((rows, C), F64)
    grad[np.arange(rows), col] = (1 / (1 + np.exp(-x)) - t) / rows
    t32 = soft_targets(masks, roi_image, matched, coords.astype(F32), F32).reshape(-1)
    accurate = int(((logits[np.arange(rows), col] > 0) == (t32.astype(np.uint8) != 0)).sum())
    return float(loss), grad, t, accurate


# ---- subdivision ------------------------------------------------------------------------------------------------------
def _axis(n, dt):
    s = np.maximum(dt(0.5) * (np.arange(2 * n).astype(dt) + dt(0.5)) - dt(0.5), dt(0))
    i0 = s.astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = s - i0.astype(dt)
    return i0, i1, dt(1) - l1, l1


def upsample2(m, dt=F64):
    """(..., H, W) -> (..., 2H, 2W): F.interpolate(scale_factor=2, mode='bilinear', align_corners=False)."""
    m = m.astype(dt)
    H, W = m.shape[-2:]
    a0, a1, la0, la1 = _axis(H, dt)
    b0, b1, lb0, lb1 = _axis(W, dt)
    top = lb0 * m[..., a0, :][..., b0] + lb1 * m[..., a0, :][..., b1]
    bot = lb0 * m[..., a1, :][..., b0] + lb1 * m[..., a1, :][..., b1]
    return np.ascontiguousarray(la0[:, None] * top + la1[:, None] * bot)      # (C order: callers write through reshaped views)


def grid_topk(u, n, dt=F32):
    """u (R, H, W) uncertainties -> indices (R, n) in our order, coords (R, n, 2) as the reference forms them: the
    steps are doubles, the sum is float32."""
    R, H, W = u.shape
    n = min(H * W, n)
    idx = np.stack([order(row.reshape(-1))[:n] for row in u]) if R else np.zeros((0, n), np.int64)
    ws, hs = 1.0 / float(W), 1.0 / float(H)
    x = dt(ws / 2.0) + (idx % W).astype(dt) * dt(ws)
    y = dt(hs / 2.0) + (idx // W).astype(dt) * dt(hs)
    return idx, np.stack([x, y], -1)


def subdivide(m, num_points, dt=F64):
    """One step on (R, H, W): the up-sampled map, and the chosen cells and their coordinates (None when skipped)."""
    up = upsample2(m, dt)
    if num_points <= 0:
        return up, None, None
    idx, coords = grid_topk(-np.abs(up), num_points)
    return up, idx, coords


def subdivision_loop(coarse, classes, point_fn, steps, num_points, one_channel, margin=0.0):
    """_forward_mask_point's inference loop.  coarse (R, C, S, S); point_fn(point coords (R, n, 2)) -> point logits
    (R, n, C).  one_channel: carry only the predicted class's map.  -> the final map ((R, H, W) of the predicted class
    either way) and the rois that were ambiguous (within `margin`) at some step."""
    R, C = coarse.shape[:2]
    ch = np.zeros(R, np.int64) if C == 1 else classes
    pick = lambda t: t[np.arange(R), ch]       # noqa: E731
    m = pick(coarse).astype(F64) if one_channel else coarse.astype(F64)
    amb = np.zeros(R, bool)
    for step in range(steps):
        m = upsample2(m)
        H, W = m.shape[-2:]
        if num_points >= 4 * H * W and step < steps - 1:
            continue
        own = m if one_channel else pick(m)
        u = -np.abs(own)
        n = min(H * W, num_points)
        amb |= ambiguous(u.reshape(R, -1), n, margin)
        idx, coords = grid_topk(u, num_points, F64)
        logits = point_fn(coords)
        flat = m.reshape(R, -1) if one_channel else m.reshape(R, C, -1)
        assert np.shares_memory(flat, m)
        for r in range(R):
            if one_channel:
                flat[r, idx[r]] = logits[r, :, ch[r]]
            else:
                flat[r][:, idx[r]] = logits[r].T
    return (m if one_channel else pick(m)), amb


# ---- the recorded cases' inputs ---------------------------------------------------------------------------------------
# name: (levels [(C, H, W, scale)], rois per image, P, coarse channels or 0)
GATHER_CASES = {
    "one": ([(5, 13, 9, 0.25)], [3, 0], 7, 5),
    "two": ([(40, 32, 32, 0.25), (40, 16, 16, 0.125)], [2, 2], 196, 5),
    "c256": ([(256, 13, 9, 0.25)], [1, 1], 1, 0),
    "c1": ([(5, 32, 32, 0.25)], [0, 2], 7, 1),
}
# name: (R, C, S, P, oversample, importance ratio)
SELECT_CASES = {
    "p8c1": (3, 1, 7, 8, 3, 0.75),
    "p8c5": (3, 5, 7, 8, 3, 0.75),
    "shipped": (2, 5, 7, 196, 3, 0.75),
    "beta1": (2, 5, 7, 8, 3, 1.0),
    "beta0": (2, 5, 7, 8, 3, 0.0),
}
# name: (per image (G, h, w) or None, rois per image, P, C)
LOSS_CASES = {
    "two": ([(3, 37, 53), (2, 20, 20)], [4, 3], 7, 5),
    "c1": ([(3, 37, 53), (2, 20, 20)], [2, 2], 7, 1),
    "empty": ([(2, 37, 53), None], [3, 0], 7, 5),
}
# name: (R, H, W, N)
SUBDIV_CASES = {
    "s4": (3, 4, 4, 10),
    "s7": (1, 7, 7, 784),
    "s14": (3, 14, 14, 784),
    "s28": (1, 28, 28, 784),
    "s112": (2, 112, 112, 784),
}


def gather_inputs(name, seed):
    levels, counts, P, cc = GATHER_CASES[name]
    rng = np.random.RandomState(seed)
    N, R = len(counts), sum(counts)
    fine = [rng.randn(N, c, h, w).astype(F32) for c, h, w, _ in levels]
    scales = [s for _, _, _, s in levels]
    ih, iw = levels[0][1] / levels[0][3], levels[0][2] / levels[0][3]
    x1, y1 = rng.uniform(-0.2 * iw, 0.7 * iw, R), rng.uniform(-0.2 * ih, 0.7 * ih, R)
    boxes = np.stack([x1, y1, x1 + rng.uniform(4, 0.6 * iw, R), y1 + rng.uniform(4, 0.6 * ih, R)], 1).astype(F32)
    points = rng.uniform(0, 1, (R, P, 2)).astype(F32)
    if P >= 7:
        points[:, 0], points[:, 1], points[:, 2] = (0.0, 0.0), (1.0, 1.0), (0.0, 1.0)
    roi_image = np.repeat(np.arange(N), counts).astype(np.int32)
    coarse = rng.randn(R, cc, 7, 7).astype(F32) if cc else None
    return fine, scales, coarse, boxes, roi_image, points


def select_inputs(name, seed):
    R, C, S, P, k, beta = SELECT_CASES[name]
    rng = np.random.RandomState(seed)
    coarse = (2 * rng.randn(R, C, S, S)).astype(F32)
    classes = rng.randint(0, C, R).astype(np.int64)
    num_uncertain = int(beta * P)
    torch.manual_seed(seed)                      # the two draws of the reference, in its order
    cand = torch.rand(R, int(P * k), 2).numpy()
    rand = torch.rand(R, P - num_uncertain, 2).numpy() if P > num_uncertain else None
    return coarse, classes, cand, rand, P, num_uncertain


def loss_inputs(name, seed):
    images, counts, P, C = LOSS_CASES[name]
    rng = np.random.RandomState(seed)
    masks = []
    for spec in images:
        if spec is None:
            masks.append(None)
            continue
        g, h, w = spec
        m = np.zeros((g, h, w), np.uint8)
        for i in range(g):       # a solid block (targets of 1.0 and just below inside, 0 outside) plus speckle
            y0, x0 = rng.randint(0, h // 2), rng.randint(0, w // 2)
            m[i, y0:y0 + h // 2, x0:x0 + w // 2] = 1
            m[i] |= (rng.uniform(size=(h, w)) < 0.1).astype(np.uint8)
        masks.append(m)
    R = sum(counts)
    roi_image = np.repeat(np.arange(len(counts)), counts).astype(np.int32)
    matched = np.array([rng.randint(0, len(masks[n])) for n in roi_image], np.int32).reshape(R)
    coords = np.zeros((R, P, 2), F32)
    for r in range(R):
        h, w = masks[roi_image[r]].shape[1:]
        coords[r, :, 0] = rng.uniform(-0.15 * w, 1.15 * w, P)       # some points outside the mask
        coords[r, :, 1] = rng.uniform(-0.15 * h, 1.15 * h, P)
        ys, xs = np.nonzero(masks[roi_image[r]][matched[r]])
        coords[r, 0] = (xs[len(xs) // 2] + 0.5, ys[len(ys) // 2] + 0.5)      # a pixel centre inside the instance
    logits = (2 * rng.randn(R * P, C)).astype(F32)
    classes = rng.randint(0, C, R).astype(np.int64)
    return logits, classes, masks, roi_image, matched, coords, P


def subdiv_inputs(name, seed):
    R, H, W, N = SUBDIV_CASES[name]
    rng = np.random.RandomState(seed)
    return (2 * rng.randn(R, H, W)).astype(F32), N


def step_points(H, W, N, last=False):
    """The reference's skip rule for the step H x W -> 2H x 2W: 0 = only up-sample."""
    return 0 if (N >= 4 * (2 * H) * (2 * W) and not last) else N


def golden():
    """The recorded reference vectors and their `meta` (bars and margins) as a dict."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointrend_reference_cases.npz"))
    return z, dict(zip([str(k) for k in z["meta_keys"]], [float(v) for v in z["meta_values"]]))
