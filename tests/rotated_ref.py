"""NumPy restatement of rotated-box IoU and NMS: the DEVICE branch of the reference's box_iou_rotated_utils.h
(what it compiles to under __HIP__ / __CUDACC__), with every fp32 operation rounded on its own and double where the
header uses double.  It is the yardstick of jtsm_amd/csrc/rotated_boxes.hip and shares no code with it.

Types, as the header has them: theta = angle * 0.01745329251 and its cos / sin are double, cast to float; the centre
shift is (float + float) / 2.0 in double, subtracted in double, stored to float; EPS = 1e-5 and the literals 1e-14,
1e-6, 1e-8 are double and the comparisons against them are made in double.  The hull: exchange sort by cross product
with the 1e-6 tie rule on `dist` computed before the sort; Graham scan comparing the two rounded products.

All functions work on K pairs at once (one row per pair) so that a few thousand pairs cost a fraction of a second;
control flow that depends on a pair is a mask.  cos / sin go through math.cos / math.sin (the C library's, as the
reference's host code calls them)."""
import math

import numpy as np

F = np.float32
EPS = 1e-5


def _f64(x):
    return x.astype(np.float64)


def _trig(angle):
    theta = _f64(angle) * 0.01745329251
    c = np.array([math.cos(t) if math.isfinite(t) else float("nan") for t in theta], dtype=np.float64)
    s = np.array([math.sin(t) if math.isfinite(t) else float("nan") for t in theta], dtype=np.float64)
    return c.astype(F) * F(0.5), s.astype(F) * F(0.5)


def _vertices(x, y, w, h, a):
    c2, s2 = _trig(a)
    p0x = (x + s2 * h) + c2 * w
    p0y = (y + c2 * h) - s2 * w
    p1x = (x - s2 * h) + c2 * w
    p1y = (y - c2 * h) - s2 * w
    p2x, p2y = F(2) * x - p0x, F(2) * y - p0y
    p3x, p3y = F(2) * x - p1x, F(2) * y - p1y
    return np.stack([p0x, p1x, p2x, p3x], 1), np.stack([p0y, p1y, p2y, p3y], 1)


def _cross(ax, ay, bx, by):
    return ax * by - bx * ay


def _dot(ax, ay, bx, by):
    return ax * bx + ay * by


def _inside(ax, ay, bx, by, vbx, vby):
    """vertices a[i] inside rectangle b (edges vb): (K,4) mask"""
    ABx, ABy, DAx, DAy = vbx[:, 0:1], vby[:, 0:1], vbx[:, 3:4], vby[:, 3:4]
    ABdotAB, ADdotAD = _dot(ABx, ABy, ABx, ABy), _dot(DAx, DAy, DAx, DAy)
    APx, APy = ax - bx[:, 0:1], ay - by[:, 0:1]
    APdotAB, APdotAD = _dot(APx, APy, ABx, ABy), -_dot(APx, APy, DAx, DAy)
    return ((_f64(APdotAB) > -EPS) & (_f64(APdotAD) > -EPS) & (_f64(APdotAB) < _f64(ABdotAB) + EPS)
            & (_f64(APdotAD) < _f64(ADdotAD) + EPS))


def iou_pairs(b1, b2):
    """IoU of b1[k] with b2[k]; b1, b2 (K,5) float32 -> (K,) float32."""
    b1, b2 = np.ascontiguousarray(b1, dtype=F).reshape(-1, 5), np.ascontiguousarray(b2, dtype=F).reshape(-1, 5)
    K = b1.shape[0]
    out = np.zeros(K, dtype=F)
    if K == 0:
        return out
    with np.errstate(all="ignore"):
        sx, sy = _f64(b1[:, 0] + b2[:, 0]) / 2.0, _f64(b1[:, 1] + b2[:, 1]) / 2.0
        x1, y1 = (_f64(b1[:, 0]) - sx).astype(F), (_f64(b1[:, 1]) - sy).astype(F)
        x2, y2 = (_f64(b2[:, 0]) - sx).astype(F), (_f64(b2[:, 1]) - sy).astype(F)
        area1, area2 = b1[:, 2] * b1[:, 3], b2[:, 2] * b2[:, 3]
        alive = ~((_f64(area1) < 1e-14) | (_f64(area2) < 1e-14))
        p1x, p1y = _vertices(x1, y1, b1[:, 2], b1[:, 3], b1[:, 4])
        p2x, p2y = _vertices(x2, y2, b2[:, 2], b2[:, 3], b2[:, 4])
        nxt = [1, 2, 3, 0]
        v1x, v1y = p1x[:, nxt] - p1x, p1y[:, nxt] - p1y
        v2x, v2y = p2x[:, nxt] - p2x, p2y[:, nxt] - p2y

        # candidates in the header's order: 16 edge crossings, 4 vertices of box 1 in box 2, 4 of box 2 in box 1
        cx, cy, ok = np.zeros((K, 24), F), np.zeros((K, 24), F), np.zeros((K, 24), bool)
        for i in range(4):
            for j in range(4):
                det = _cross(v2x[:, j], v2y[:, j], v1x[:, i], v1y[:, i])
                skip = np.abs(_f64(det)) <= 1e-14
                v12x, v12y = p2x[:, j] - p1x[:, i], p2y[:, j] - p1y[:, i]
                t1 = _cross(v2x[:, j], v2y[:, j], v12x, v12y) / det
                t2 = _cross(v1x[:, i], v1y[:, i], v12x, v12y) / det
                hit = (~skip & (_f64(t1) > -EPS) & (_f64(t1) < 1.0 + EPS) & (_f64(t2) > -EPS) & (_f64(t2) < 1.0 + EPS))
                cx[:, 4 * i + j] = p1x[:, i] + v1x[:, i] * t1
                cy[:, 4 * i + j] = p1y[:, i] + v1y[:, i] * t1
                ok[:, 4 * i + j] = hit
        cx[:, 16:20], cy[:, 16:20], ok[:, 16:20] = p1x, p1y, _inside(p1x, p1y, p2x, p2y, v2x, v2y)
        cx[:, 20:24], cy[:, 20:24], ok[:, 20:24] = p2x, p2y, _inside(p2x, p2y, p1x, p1y, v1x, v1y)
        pack = np.argsort(~ok, axis=1, kind="stable")
        qx, qy = np.take_along_axis(cx, pack, 1), np.take_along_axis(cy, pack, 1)
        num = ok.sum(1)
        alive &= num > 2
        rows = np.arange(K)
        nmax = int(num[alive].max()) if alive.any() else 0

        # lowest-then-leftmost point, shift, swap it to the front
        t = np.zeros(K, dtype=np.int64)
        for i in range(1, nmax):
            ty, tx = qy[rows, t], qx[rows, t]
            better = (i < num) & ((qy[:, i] < ty) | ((qy[:, i] == ty) & (qx[:, i] < tx)))
            t[better] = i
        qx, qy = qx - qx[rows, t][:, None], qy - qy[rows, t][:, None]
        for q in (qx, qy):
            tmp = q[:, 0].copy()
            q[:, 0] = q[rows, t]
            q[rows, t] = tmp
        dist = _dot(qx, qy, qx, qy)

        # the device branch's exchange sort
        for i in range(1, nmax - 1):
            for j in range(i + 1, nmax):
                cp = _f64(_cross(qx[:, i], qy[:, i], qx[:, j], qy[:, j]))
                swap = (j < num) & ((cp < -1e-6) | ((np.abs(cp) < 1e-6) & (dist[:, i] > dist[:, j])))
                if swap.any():
                    for arr in (qx, qy, dist):
                        tmp = arr[swap, i].copy()
                        arr[swap, i] = arr[swap, j]
                        arr[swap, j] = tmp

        # first point away from the start
        k = num.astype(np.int64)
        for i in range(nmax - 1, 0, -1):
            k[(i < num) & (_f64(dist[:, i]) > 1e-8)] = i
        alive &= k < num
        kc = np.minimum(k, 23)
        qx[:, 1], qy[:, 1] = qx[rows, kc], qy[rows, kc]
        m = np.full(K, 2, dtype=np.int64)
        for i in range(2, nmax):
            act = alive & (i > k) & (i < num)
            if not act.any():
                continue
            while True:
                bx, by = qx[rows, np.maximum(m - 2, 0)], qy[rows, np.maximum(m - 2, 0)]
                q1x, q1y = qx[:, i] - bx, qy[:, i] - by
                q2x, q2y = qx[rows, m - 1] - bx, qy[rows, m - 1] - by
                pop = act & (m > 1) & (q1x * q2y >= q2x * q1y)
                if not pop.any():
                    break
                m[pop] -= 1
            r = rows[act]
            xi, yi = qx[r, i].copy(), qy[r, i].copy()
            qx[r, m[r]], qy[r, m[r]] = xi, yi
            m[act] += 1
        alive &= m > 2
        area = np.zeros(K, dtype=F)
        for i in range(1, nmax - 1):
            act = alive & (i < m - 1)
            if not act.any():
                continue
            ax, ay = qx[:, i] - qx[:, 0], qy[:, i] - qy[:, 0]
            bx, by = qx[:, i + 1] - qx[:, 0], qy[:, i + 1] - qy[:, 0]
            area = np.where(act, area + np.abs(_cross(ax, ay, bx, by)), area)
        inter = (_f64(area) / 2.0).astype(F)
        iou = inter / ((area1 + area2) - inter)
        out = np.where(alive, iou, F(0)).astype(F)
    return out


def iou_matrix(boxes1, boxes2, chunk=65536):
    """(N,5), (M,5) -> (N,M) float32"""
    boxes1, boxes2 = np.asarray(boxes1, dtype=F).reshape(-1, 5), np.asarray(boxes2, dtype=F).reshape(-1, 5)
    N, M = boxes1.shape[0], boxes2.shape[0]
    out = np.zeros(N * M, dtype=F)
    ii, jj = np.divmod(np.arange(N * M), max(M, 1))
    for s in range(0, N * M, chunk):
        out[s:s + chunk] = iou_pairs(boxes1[ii[s:s + chunk]], boxes2[jj[s:s + chunk]])
    return out.reshape(N, M)


def score_order(scores):
    """descending score, equal scores by lower index"""
    return np.argsort(-np.asarray(scores, dtype=np.float64), kind="stable")


def greedy_nms(order, iou_row, threshold, strict=True, compared=None):
    """The greedy pass over `order`; iou_row(i, js) -> IoU of element i with elements js.  strict: suppress on
    iou > threshold (the reference's CUDA kernel), else on >= (its CPU kernel).  `compared` (a list) collects every
    IoU the pass looks at."""
    order = np.asarray(order)
    suppressed = np.zeros(order.shape[0], dtype=bool)
    keep = []
    for a in range(order.shape[0]):
        if suppressed[a]:
            continue
        keep.append(int(order[a]))
        later = np.nonzero(~suppressed[a + 1:])[0] + a + 1
        if later.size == 0:
            continue
        v = np.asarray(iou_row(int(order[a]), order[later]))
        if compared is not None:
            compared.append(v)
        suppressed[later[(v > threshold) if strict else (v >= threshold)]] = True
    return np.asarray(keep, dtype=np.int64)


def nms(boxes, scores, threshold, compared=None):
    """nms_rotated with `>`: keep indices in decreasing score order."""
    boxes = np.asarray(boxes, dtype=F).reshape(-1, 5)
    return greedy_nms(score_order(scores), lambda i, js: iou_pairs(np.repeat(boxes[i:i + 1], len(js), 0), boxes[js]),
                      threshold, True, compared)


def batched_nms(boxes, scores, idxs, threshold, compared=None):
    """Per-class NMS on the un-offset boxes; keep indices in decreasing score order."""
    boxes, scores, idxs = np.asarray(boxes, dtype=F).reshape(-1, 5), np.asarray(scores), np.asarray(idxs)
    keep = []
    for c in np.unique(idxs):
        sel = np.nonzero(idxs == c)[0]
        keep.append(sel[nms(boxes[sel], scores[sel], threshold, compared)])
    keep = np.concatenate(keep) if keep else np.zeros(0, dtype=np.int64)
    return keep[np.argsort(-scores[keep].astype(np.float64), kind="stable")] if keep.size else keep


def clustered_boxes(n, seed, jitter=1.0, with_scores=True, classes=1):
    """The input recipe: 6 base rectangles (centres in [50, 350], sides in [20, 100], angle in [-180, 180)), every box
    one of them with its centre jittered by sigma = 8 px, each side by +-12.5 % and the angle by sigma = 10 degrees
    (all three scaled by `jitter`); scores uniform without ties (None without with_scores).  -> boxes (n,5) f32, scores (n) f32, idxs (n) i64"""
    rng = np.random.RandomState(seed)
    base = np.concatenate([rng.uniform(50, 350, (6, 2)), rng.uniform(20, 100, (6, 2)), rng.uniform(-180, 180, (6, 1))], 1)
    which = rng.randint(0, 6, n)
    b = base[which]
    b[:, 0:2] += rng.normal(0, 8.0 * jitter, (n, 2))
    b[:, 2:4] *= 1.0 + rng.uniform(-0.125 * jitter, 0.125 * jitter, (n, 2))
    b[:, 4] += rng.normal(0, 10.0 * jitter, n)
    scores = None
    if with_scores:
        scores = rng.uniform(0.0, 1.0, n).astype(F)
        assert np.unique(scores).size == n, "tied scores"
    idxs = rng.randint(0, classes, n).astype(np.int64)
    return b.astype(F), scores, idxs


def known_answer_cases():
    """The RNG-free known answers of the reference's tests/structures/test_rotated_boxes.py:
    (name, boxes1, boxes2, expected (N,M) or None).  `extreme` has no expected matrix: its IoUs must be >= 0."""
    s2 = math.sqrt(2)
    unit = [0.5, 0.5, 1.0, 1.0, 0.0]
    many1 = [[5 + 20 * i, 5 + 20 * i, 10, 10, 0] for i in range(100)]
    many2 = [[5 + 20 * i, 5 + 20 * i, 10, 1 + 9 * i / 200, 0] for i in range(200)]
    many = np.zeros((100, 200))
    for i in range(100):
        many[i, i] = (1 + 9 * i / 200) / 10.0
    cases = [
        ("0_dim_a", np.zeros((0, 5)), np.full((10, 5), 0.5), np.zeros((0, 10))),
        ("0_dim_b", np.full((10, 5), 0.5), np.zeros((0, 5)), np.zeros((10, 0))),
        ("half_overlap", [unit], [[0.25, 0.5, 0.5, 1.0, 0.0]], [[0.5]]),
        ("precision", [[565, 565, 10, 10.0, 0]], [[565, 565, 10, 8.3, 0]], [[8.3 / 10.0]]),
        ("extreme", [[160.0, 153.0, 230.0, 23.0, -37.0]],
         [[-1.117407639806935e17, 1.3858420478349148e18, 1000.0000610351562, 1000.0000610351562, 1612.0]], None),
        ("issue_2154", [[296.6620178222656, 458.73883056640625, 23.515729904174805, 47.677001953125, 0.08795166015625]],
         [[296.66201, 458.73882000000003, 23.51573, 47.67702, 0.087951]], [[1.0]]),
        ("issue_2167", [[2563.74462890625, 1436.7901611328125, 2174.703369140625, 214.09500122070312, 115.11834716796875]],
         [[2563.74462890625, 1436.790283203125, 2174.702880859375, 214.0949554443359375, 115.11835479736328125]], [[1.0]]),
        ("0_degree", [unit, unit],
         [unit, [0.25, 0.5, 0.5, 1.0, 0.0], [0.5, 0.25, 1.0, 0.5, 0.0], [0.25, 0.25, 0.5, 0.5, 0.0],
          [0.75, 0.75, 0.5, 0.5, 0.0], [1.0, 1.0, 1.0, 1.0, 0.0]],
         [[1.0, 0.5, 0.5, 0.25, 0.25, 0.25 / (2 - 0.25)]] * 2),
        ("45_degrees", [[1, 1, s2, s2, 45], [1, 1, 2 * s2, 2 * s2, -45]], [[1, 1, 2, 2, 0]], [[0.5], [0.5]]),
        ("orthogonal", [[5, 5, 10, 6, 55]], [[5, 5, 10, 6, -35]], [[(6.0 * 6.0) / (6.0 * 6.0 + 4.0 * 6.0 + 4.0 * 6.0)]]),
        ("large_close_boxes", [[299.5, 417.370422, 600.0, 364.259186, 27.1828]],
         [[299.5, 417.370422, 600.0, 364.259155, 27.1828]], [[364.259155 / 364.259186]]),
        ("many_boxes", many1, many2, many),
        ("issue1207_simplified", [[3, 3, 8, 2, -45.0]], [[6, 0, 8, 2, -45.0]], [[0.0]]),
        ("issue1207", [[160.0, 153.0, 230.0, 23.0, -37.0]], [[190.0, 127.0, 80.0, 21.0, -46.0]], [[0.0]]),
    ]
    return [(n, np.asarray(a, dtype=F).reshape(-1, 5), np.asarray(b, dtype=F).reshape(-1, 5),
             None if e is None else np.asarray(e, dtype=F)) for n, a, b, e in cases]


def allclose_default(got, want):
    """torch.allclose's defaults: |got - want| <= 1e-8 + 1e-5 * |want|"""
    return bool(np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= 1e-8 + 1e-5 * np.abs(want.astype(np.float64))))
