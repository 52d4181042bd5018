"""CPU restatement of ROILoopPool's CUDA contract (projects/WSL/wsl/layers/csrc/ROILoopPool/ROILoopPool_cuda.cu):
forward RoILoopPoolForward :10-205 with the host wrapper's ratio 1.8 (:309), backward RoILoopPoolBackward :207-249.

Geometry in float32, each step rounded on its own (numpy float32 scalars): the reading the HIP kernel implements
(contraction off).  `fused=True` gives the other reading of `rois_outer_w - rois_w`, i.e. fma(w, 1.8f, -w) rounded
once, which a CUDA build may produce; it exists to list the boxes on which the two readings part.
Lives under tests/ (oracle/ is frozen)."""
import numpy as np

F = np.float32
RATIO = F(1.8)     # a double literal passed to the kernel's float parameter


def roundf(v):
    """C roundf: half away from zero (torch.round / np.round are half-to-even)."""
    v = F(v)
    t = np.trunc(v)
    if abs(F(v - t)) >= F(0.5):
        t = t + np.sign(v)
    return int(t)


def _outer_residual(w, fused):
    if fused:   # w * ratio - w as one fused multiply-add: exact in double (48-bit product), then rounded once
        return F(np.float64(w) * np.float64(RATIO) - np.float64(w))
    return F(F(w * RATIO) - w)


def geometry(roi, scale, H, W, fused=False):
    """Integer rectangles (x0, y0, x1, y1) of the box, the inner box and the outer box, and the clamped float outer
    box (ROILoopPool_cuda.cu:34-75, 77-87, 141-152)."""
    scale = F(scale)
    x1, y1, x2, y2 = (F(v) for v in roi[1:5])
    rw, rh = F(x2 - x1), F(y2 - y1)
    iw, ih = F(rw / RATIO), F(rh / RATIO)
    irw, irh = F(rw - iw), F(rh - ih)
    orw, orh = _outer_residual(rw, fused), _outer_residual(rh, fused)
    bx, by = F(1.0 * W / np.float64(scale)), F(1.0 * H / np.float64(scale))

    def cl(v, hi):
        return F(min(max(F(v), F(0)), hi))

    inner = (cl(x1 + F(irw / F(2)), bx), cl(y1 + F(irh / F(2)), by), cl(x2 - F(irw / F(2)), bx), cl(y2 - F(irh / F(2)), by))
    outer = (cl(x1 - F(orw / F(2)), bx), cl(y1 - F(orh / F(2)), by), cl(x2 + F(orw / F(2)), bx), cl(y2 + F(orh / F(2)), by))
    rect = lambda q: tuple(roundf(F(v * scale)) for v in q)   # noqa: E731
    return {"box": rect((x1, y1, x2, y2)), "inner": rect(inner), "outer": rect(outer), "outer_f": outer}


def bins(rect, P, size, axis):
    """[start, end) of every bin along one axis, clipped to the map (ROILoopPool_cuda.cu:89-104)."""
    s, e = (rect[0], rect[2]) if axis == "x" else (rect[1], rect[3])
    n = max(e - s + 1, 1)
    b = F(F(n) / F(P))
    out = []
    for p in range(P):
        lo = int(np.floor(F(F(p) * b))) + s
        hi = int(np.ceil(F(F(p + 1) * b))) + s
        out.append((min(max(lo, 0), size), min(max(hi, 0), size)))
    return out


def _pool(plane, hs, he, ws, we, keep):
    """Max over a bin of a (C, H, W) plane with the reference's scan: maxima start at 0, argmax -1, strict '>' in
    h-outer / w-inner order — the first cell holding the bin's maximum wins, if that maximum is > 0.
    keep: (he-hs, we-ws) bool, the cells that count."""
    C, _, W = plane.shape
    val = np.zeros(C, np.float32)
    arg = np.full(C, -1, np.int32)
    if he <= hs or we <= ws or not keep.any():
        return val, arg
    blk = np.where(keep[None], plane[:, hs:he, ws:we], -np.inf).reshape(C, -1)
    k = blk.argmax(axis=1)
    m = blk[np.arange(C), k]
    hit = m > 0
    val[hit] = m[hit]
    hh, ww = np.divmod(k, we - ws)
    arg[hit] = ((hh + hs) * W + ww + ws)[hit].astype(np.int32)
    return val, arg


def forward(x, rois, scale, PH, PW, fused=False):
    """x (B, C, H, W) float32, rois (R, 5) -> output (3R, C, PH, PW) float32, argmax int32."""
    x = np.asarray(x, np.float32)
    rois = np.asarray(rois, np.float32)
    B, C, H, W = x.shape
    R = rois.shape[0]
    out = np.zeros((3 * R, C, PH, PW), np.float32)
    arg = np.full((3 * R, C, PH, PW), -1, np.int32)
    for n in range(R):
        if not 0 <= int(rois[n][0]) < B:                # (a roi naming no image pools nothing: 0 / -1)
            continue
        g = geometry(rois[n], scale, H, W, fused)
        plane = x[int(rois[n][0])]
        box, inner, outer = g["box"], g["inner"], g["outer"]
        by, bxs = bins(box, PH, H, "y"), bins(box, PW, W, "x")
        oy, oxs = bins(outer, PH, H, "y"), bins(outer, PW, W, "x")
        for ph in range(PH):
            for pw in range(PW):
                hs, he = by[ph]
                ws, we = bxs[pw]
                hh = np.arange(hs, he)[:, None]
                ww = np.arange(ws, we)[None, :]
                allc = np.ones((max(he - hs, 0), max(we - ws, 0)), bool)
                out[n, :, ph, pw], arg[n, :, ph, pw] = _pool(plane, hs, he, ws, we, allc)
                inside = (hh > inner[1]) & (hh < inner[3]) & (ww > inner[0]) & (ww < inner[2])
                out[R + n, :, ph, pw], arg[R + n, :, ph, pw] = _pool(plane, hs, he, ws, we, ~inside)
                hs, he = oy[ph]
                ws, we = oxs[pw]
                hh = np.arange(hs, he)[:, None]
                ww = np.arange(ws, we)[None, :]
                inside = (hh > box[1]) & (hh < box[3]) & (ww > box[0]) & (ww < box[2])
                out[2 * R + n, :, ph, pw], arg[2 * R + n, :, ph, pw] = _pool(plane, hs, he, ws, we, ~inside)
    return out, arg


def backward(grad, rois, argmax, B, C, H, W):
    """Scatter-add of RoILoopPoolBackward: grad_in[b, c, argmax] += grad[n, c, ph, pw], image of row n from
    rois[n % R].  Accumulated in float64, returned as float32."""
    grad = np.asarray(grad, np.float64)
    argmax = np.asarray(argmax)
    rois = np.asarray(rois, np.float32)
    R = rois.shape[0]
    gin = np.zeros((B, C, H * W), np.float64)
    n3 = argmax.shape[0]
    for n in range(n3):
        b = int(rois[n % R][0])
        if not 0 <= b < B:
            continue
        a = argmax[n].reshape(C, -1)
        g = grad[n].reshape(C, -1)
        for c in range(C):
            ok = a[c] >= 0
            np.add.at(gin[b, c], a[c][ok], g[c][ok])
    return gin.reshape(B, C, H, W).astype(np.float32)
