"""NumPy restatement of the keypoint path, written from the reference's text (detectron2/structures/keypoints.py,
detectron2/modeling/roi_heads/keypoint_head.py and roi_heads.py:77-121) and from the definition of
F.interpolate(mode="bicubic" / "bilinear", align_corners=False):

  targets / valid                     in fp32, operation for operation
  decode (heatmaps_to_keypoints)      the up-sampled map in fp64, horizontal sums first; the final coordinates in the
                                      reference's fp32 arithmetic
  loss and its gradient               in fp64
  ConvTranspose2d(4, stride 2, padding 1) and the x2 bilinear, with their adjoints, in fp64
  select_proposals_with_visible_keypoints

and the input generators of the keypoint tests, on numpy.random.RandomState so that any machine regenerates the same
inputs from a seed."""
import numpy as np

A = -0.75


# ---- generators -----------------------------------------------------------------------------------------------------
def blob_maps(rs, R, K, S):
    """A Gaussian peak of height 8 and sigma S / 14 at a random place, plus 0.3 x normal noise."""
    cy, cx = rs.uniform(0, S, (R, K, 1, 1)), rs.uniform(0, S, (R, K, 1, 1))
    yy, xx = np.arange(S)[None, None, :, None] + 0.5, np.arange(S)[None, None, None, :] + 0.5
    sig = S / 14.0
    m = 8.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sig * sig)) + 0.3 * rs.standard_normal((R, K, S, S))
    return m.astype(np.float32)


def plain_maps(rs, R, K, S):
    return (2.0 * rs.standard_normal((R, K, S, S))).astype(np.float32)


def boxes(rs, R, wmax, wmin=0.5):
    """Sides log-uniform in [wmin, wmax], corners uniform in [0, 200)."""
    w = np.exp(rs.uniform(np.log(wmin), np.log(wmax), R))
    h = np.exp(rs.uniform(np.log(wmin), np.log(wmax), R))
    x1, y1 = rs.uniform(0, 200, R), rs.uniform(0, 200, R)
    return np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32)


def make_maps(kind, seed, R, K, S):
    return {"blob": blob_maps, "plain": plain_maps}[kind](np.random.RandomState(seed), R, K, S)


def keypoints_for(rs, rois, K, S):
    """(N, K, 3) for rois (N, 4): inside points, points on x2 / y2, points exactly on cell edges
    x1 + j (x2 - x1) / S, points outside, v = 0 (with x = y = 0) and v in {1, 2}."""
    rois = rois.astype(np.float32)
    N = rois.shape[0]
    x1, y1, x2, y2 = [rois[:, i:i + 1] for i in range(4)]
    kp = np.zeros((N, K, 3), np.float32)
    u, v = rs.uniform(0, 1, (N, K)).astype(np.float32), rs.uniform(0, 1, (N, K)).astype(np.float32)
    kp[:, :, 0] = x1 + u * (x2 - x1)
    kp[:, :, 1] = y1 + v * (y2 - y1)
    kp[:, :, 2] = rs.randint(1, 3, (N, K))
    which = (np.arange(N)[:, None] * 3 + np.arange(K)[None, :]) % 8
    j = rs.randint(0, S + 1, (N, K)).astype(np.float32)
    edge_x = (x1 + j * (x2 - x1) / np.float32(S)).astype(np.float32)
    edge_y = (y1 + j * (y2 - y1) / np.float32(S)).astype(np.float32)
    kp[:, :, 0] = np.where(which == 1, np.broadcast_to(x2, (N, K)), kp[:, :, 0])
    kp[:, :, 1] = np.where(which == 2, np.broadcast_to(y2, (N, K)), kp[:, :, 1])
    kp[:, :, 0] = np.where(which == 3, edge_x, kp[:, :, 0])
    kp[:, :, 1] = np.where(which == 4, edge_y, kp[:, :, 1])
    kp[:, :, 0] = np.where(which == 5, np.broadcast_to(x2 + (x2 - x1) * np.float32(0.5), (N, K)), kp[:, :, 0])   # outside
    kp[:, :, 1] = np.where(which == 6, np.broadcast_to(y1 - np.float32(3.0), (N, K)), kp[:, :, 1])               # outside
    kp[which == 7] = 0                                                                                            # v = 0
    return kp


# ---- targets --------------------------------------------------------------------------------------------------------
def keypoints_to_heatmap(keypoints, rois, S):
    """int64 targets (N, K), int64 valid (N, K); all arithmetic in fp32."""
    kp, rois = np.asarray(keypoints, np.float32), np.asarray(rois, np.float32)
    if rois.size == 0:
        return np.zeros(kp.shape[:2], np.int64), np.zeros(kp.shape[:2], np.int64)
    fs = np.float32(S)
    with np.errstate(divide="ignore", invalid="ignore"):
        # `heatmap_size / tensor` is Tensor.__rtruediv__: tensor.reciprocal() * heatmap_size, two roundings
        sx = ((np.float32(1) / (rois[:, 2] - rois[:, 0])) * fs)[:, None]
        sy = ((np.float32(1) / (rois[:, 3] - rois[:, 1])) * fs)[:, None]
        x, y = kp[..., 0], kp[..., 1]
        xb, yb = x == rois[:, 2][:, None], y == rois[:, 3][:, None]
        cx = np.floor(((x - rois[:, 0][:, None]) * sx).astype(np.float32))
        cy = np.floor(((y - rois[:, 1][:, None]) * sy).astype(np.float32))
    cx = np.where(xb, fs - 1, cx)
    cy = np.where(yb, fs - 1, cy)
    with np.errstate(invalid="ignore"):
        ok = (cx >= 0) & (cy >= 0) & (cx < fs) & (cy < fs) & (kp[..., 2] > 0)
    cxi = np.where(ok, cx, 0).astype(np.int64)
    cyi = np.where(ok, cy, 0).astype(np.int64)
    return (cyi * S + cxi) * ok, ok.astype(np.int64)


# ---- decode ---------------------------------------------------------------------------------------------------------
def _cubic(t):
    a, b = t + 1.0, 1.0 - t
    d = b + 1.0
    return np.stack([((A * a - 5 * A) * a + 8 * A) * a - 4 * A, ((A + 2) * t - (A + 3)) * t * t + 1,
                     ((A + 2) * b - (A + 3)) * b * b + 1, ((A * d - 5 * A) * d + 8 * A) * d - 4 * A], -1)


def _taps(n_in, n_out):
    """(n_out, 4) clamped source indices and (n_out, 4) coefficients of the bicubic resize along one axis."""
    src = (n_in / float(n_out)) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5
    f = np.floor(src)
    idx = np.clip(f[:, None].astype(np.int64) + np.arange(-1, 3)[None, :], 0, n_in - 1)
    return idx, _cubic(src - f)


def bicubic_resize(m, oh, ow):
    """m (..., S, S) float64 -> (..., oh, ow): the four-tap horizontal sums first, then the vertical combination."""
    m = np.asarray(m, np.float64)
    ix, cx = _taps(m.shape[-1], ow)
    iy, cy = _taps(m.shape[-2], oh)
    hs = sum(m[..., :, ix[:, j]] * cx[:, j] for j in range(4))                       # (..., S, ow)
    return sum(hs[..., iy[:, i], :] * cy[:, i][:, None] for i in range(4))           # (..., oh, ow)


def roi_sizes(rois):
    """fp32, as the reference: w = max(x2 - x1, 1), ceil, and the corrections w / ceil(w)."""
    rois = np.asarray(rois, np.float32)
    w = np.maximum(rois[:, 2] - rois[:, 0], np.float32(1))
    h = np.maximum(rois[:, 3] - rois[:, 1], np.float32(1))
    wc, hc = np.ceil(w), np.ceil(h)
    return w, h, wc.astype(np.int64), hc.astype(np.int64), (w / wc).astype(np.float32), (h / hc).astype(np.float32)


def heatmaps_to_keypoints(maps, rois, margin=None, want_maps=False):
    """out (R, K, 4) float64 = x, y (exact fp32 values), logit, score; with `margin`, also the (R, K) flags of the
    AMBIGUOUS rows: the two largest up-sampled values lie within `margin` of each other.  want_maps: also the list of
    (K, oh, ow) fp64 up-sampled maps."""
    maps, rois = np.asarray(maps, np.float32), np.asarray(rois, np.float32)
    R, K = maps.shape[:2]
    _, _, ow, oh, corr_x, corr_y = roi_sizes(rois)
    out = np.zeros((R, K, 4), np.float64)
    amb = np.zeros((R, K), bool)
    ups = []
    for r in range(R):
        up = bicubic_resize(maps[r], int(oh[r]), int(ow[r]))
        flat = up.reshape(K, -1)
        pos = flat.argmax(1)
        mx = flat[np.arange(K), pos]
        if margin is not None and flat.shape[1] > 1:
            second = np.partition(flat, -2, axis=1)[:, -2]
            amb[r] = mx - second <= margin
        xi, yi = pos % ow[r], pos // ow[r]
        out[r, :, 0] = (xi.astype(np.float32) + np.float32(0.5)) * corr_x[r] + rois[r, 0]
        out[r, :, 1] = (yi.astype(np.float32) + np.float32(0.5)) * corr_y[r] + rois[r, 1]
        out[r, :, 2] = mx
        out[r, :, 3] = 1.0 / np.exp(maps[r].astype(np.float64).reshape(K, -1) - mx[:, None]).sum(1)
        if want_maps:
            ups.append(up)
    res = (out,) + ((amb,) if margin is not None else ()) + ((ups,) if want_maps else ())
    return res if len(res) > 1 else out


def pixel_of(xy, rois):
    """The integer pixel (xi, yi) of decoded fp32 points (R, K, 2) in their rois' up-sampled maps."""
    rois = np.asarray(rois, np.float32)
    _, _, ow, oh, corr_x, corr_y = roi_sizes(rois)
    xi = np.rint((np.asarray(xy[..., 0], np.float64) - rois[:, None, 0]) / corr_x[:, None] - 0.5).astype(np.int64)
    yi = np.rint((np.asarray(xy[..., 1], np.float64) - rois[:, None, 1]) / corr_y[:, None] - 0.5).astype(np.int64)
    return np.clip(xi, 0, ow[:, None] - 1), np.clip(yi, 0, oh[:, None] - 1)


def value_at(maps, rois, xi, yi):
    """fp64 up-sampled value of every (roi, keypoint) map at pixel (xi, yi) (R, K), without the whole map."""
    maps = np.asarray(maps, np.float64)
    R, K, S, _ = maps.shape
    _, _, ow, oh, _, _ = roi_sizes(rois)
    out = np.zeros((R, K))
    for r in range(R):
        ix, cx = _taps(S, int(ow[r]))
        iy, cy = _taps(S, int(oh[r]))
        for k in range(K):
            patch = maps[r, k][np.ix_(iy[yi[r, k]], ix[xi[r, k]])]                   # (4, 4)
            out[r, k] = ((patch * cx[xi[r, k]][None, :]).sum(1) * cy[yi[r, k]]).sum()
    return out


# ---- loss -----------------------------------------------------------------------------------------------------------
def keypoint_loss(logits, targets, valid, normalizer=None):
    """(loss, d loss / d logits) in fp64."""
    x = np.asarray(logits, np.float64)
    N, K, S, _ = x.shape
    rows = x.reshape(N * K, S * S)
    t, v = np.asarray(targets).reshape(-1).astype(np.int64), np.asarray(valid).reshape(-1).astype(bool)
    grad = np.zeros_like(rows)
    if not v.any():
        return 0.0, grad.reshape(x.shape)
    m = rows.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(rows - m).sum(1))
    per_row = lse - rows[np.arange(rows.shape[0]), t]
    denom = float(v.sum()) if normalizer is None or normalizer <= 0 else float(normalizer)
    p = np.exp(rows - lse[:, None])
    p[np.arange(rows.shape[0]), t] -= 1.0
    grad[v] = p[v] / denom
    return float(per_row[v].sum() / denom), grad.reshape(x.shape)


# ---- head tail: ConvTranspose2d(C, K, 4, stride 2, padding 1) and the x2 bilinear -------------------------------------
def conv_transpose4x4(x, w, b):
    """x (R, C, H, W), w (C, K, 4, 4), b (K,) -> (R, K, 2H, 2W): out[2 i - 1 + ky] += x[i] w[ky]."""
    x, w, b = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64)
    R, C, H, W = x.shape
    P = np.zeros((R, w.shape[1], 2 * H + 2, 2 * W + 2))
    for ky in range(4):
        for kx in range(4):
            P[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += np.einsum("rcij,ck->rkij", x, w[:, :, ky, kx])
    return P[:, :, 1:-1, 1:-1] + b[None, :, None, None]


def conv_transpose4x4_grads(x, w, g):
    """Gradients (dx, dw, db) for the upstream gradient g (R, K, 2H, 2W)."""
    x, w, g = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(g, np.float64)
    R, C, H, W = x.shape
    P = np.pad(g, ((0, 0), (0, 0), (1, 1), (1, 1)))
    dx, dw = np.zeros_like(x), np.zeros_like(w)
    for ky in range(4):
        for kx in range(4):
            s = P[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2]
            dx += np.einsum("rkij,ck->rcij", s, w[:, :, ky, kx])
            dw[:, :, ky, kx] = np.einsum("rcij,rkij->ck", x, s)
    return dx, dw, g.sum((0, 2, 3))


def bilinear_matrix(n):
    """(2n, n): F.interpolate(scale_factor=2, mode="bilinear", align_corners=False) along one axis."""
    B = np.zeros((2 * n, n))
    for d in range(2 * n):
        s = max(0.5 * (d + 0.5) - 0.5, 0.0)
        i0 = int(np.floor(s))
        i1 = min(i0 + 1, n - 1)
        B[d, i0] += 1.0 - (s - i0)
        B[d, i1] += s - i0
    return B


def bilinear_x2(u):
    u = np.asarray(u, np.float64)
    return np.einsum("ya,rkab,xb->rkyx", bilinear_matrix(u.shape[2]), u, bilinear_matrix(u.shape[3]))


def bilinear_x2_grad(g):
    g = np.asarray(g, np.float64)
    return np.einsum("ya,rkyx,xb->rkab", bilinear_matrix(g.shape[2] // 2), g, bilinear_matrix(g.shape[3] // 2))


def head_tail(x, w, b):
    """score_lowres + interpolate: (R, C, H, W) -> (R, K, 4H, 4W)."""
    return bilinear_x2(conv_transpose4x4(x, w, b))


def head_tail_grads(x, w, g):
    return conv_transpose4x4_grads(x, w, bilinear_x2_grad(g))


# ---- proposal selection ---------------------------------------------------------------------------------------------
def select_proposals_with_visible_keypoints(boxes, keypoints):
    """Indices of the proposals (boxes (P, 4), keypoints (P, K, 3)) with a labelled keypoint (v >= 1) inside the box,
    edges included."""
    boxes, kp = np.asarray(boxes), np.asarray(keypoints)
    xs, ys, vis = kp[:, :, 0], kp[:, :, 1], kp[:, :, 2] >= 1
    inside = (xs >= boxes[:, None, 0]) & (xs <= boxes[:, None, 2]) & (ys >= boxes[:, None, 1]) & (ys <= boxes[:, None, 3])
    return np.nonzero((inside & vis).any(1))[0]
