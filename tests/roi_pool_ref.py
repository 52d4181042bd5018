"""CPU restatement of the plain ROI max-pool (the contract jtsm_amd/csrc/roi_pool.hip states; the reference reaches it
as torchvision.ops.RoIPool, projects/WSL/wsl/modeling/poolers.py:6,183-186).

rois (R, 5) = (b, x1, y1, x2, y2).  Integer rectangle = roundf(coord * scale) in float32, half away from zero;
roi_w = max(x_end - x_start + 1, 1); bin = float32(roi_w) / PW; bin p covers [floor(p*bin), ceil((p+1)*bin)) + start,
clipped to the map.  An empty bin gives 0 / -1; otherwise the first cell (h outer, w inner) holding the bin's maximum
wins, provided it is above -FLT_MAX.  Lives under tests/ (oracle/ is frozen)."""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max


def roundf(v):
    """C roundf: half away from zero."""
    v = F(v)
    t = np.trunc(v)
    if abs(F(v - t)) >= F(0.5):
        t = t + np.sign(v)
    return int(t)


def rect(roi, scale):
    scale = F(scale)
    return tuple(roundf(F(F(v) * scale)) for v in roi[1:5])


def bins(start, end, P, size):
    """Clipped [lo, hi) of every bin along one axis."""
    b = F(F(max(end - start + 1, 1)) / F(P))
    out = []
    for p in range(P):
        lo = int(np.floor(F(F(p) * b))) + start
        hi = int(np.ceil(F(F(p + 1) * b))) + start
        out.append((min(max(lo, 0), size), min(max(hi, 0), size)))
    return out


def forward(x, rois, scale, PH, PW):
    """x (B, C, H, W) float32, rois (R, 5) -> output (R, C, PH, PW) float32, argmax int32."""
    x = np.asarray(x, np.float32)
    rois = np.asarray(rois, np.float32)
    B, C, H, W = x.shape
    R = rois.shape[0]
    out = np.zeros((R, C, PH, PW), np.float32)
    arg = np.full((R, C, PH, PW), -1, np.int32)
    for n in range(R):
        b = int(rois[n][0])
        if not 0 <= b < B:
            continue
        x0, y0, x1, y1 = rect(rois[n], scale)
        by, bx = bins(y0, y1, PH, H), bins(x0, x1, PW, W)
        for ph, (hs, he) in enumerate(by):
            for pw, (ws, we) in enumerate(bx):
                if he <= hs or we <= ws:
                    continue
                blk = x[b, :, hs:he, ws:we].reshape(C, -1)
                k = blk.argmax(axis=1)                      # first maximum in h-outer / w-inner order
                m = blk[np.arange(C), k]
                hit = m > -FLT_MAX
                hh, ww = np.divmod(k, we - ws)
                out[n, :, ph, pw] = np.where(hit, m, -FLT_MAX)
                arg[n, :, ph, pw] = np.where(hit, (hh + hs) * W + ww + ws, -1)
    return out, arg


def backward(grad, rois, argmax, B, C, H, W):
    """grad_in[b, c, argmax] += grad[n, c, ph, pw] wherever argmax >= 0; accumulated in float64, returned float32."""
    grad = np.asarray(grad, np.float64)
    argmax = np.asarray(argmax)
    rois = np.asarray(rois, np.float32)
    gin = np.zeros((B, C, H * W), np.float64)
    for n in range(argmax.shape[0]):
        b = int(rois[n][0])
        if not 0 <= b < B:
            continue
        a = argmax[n].reshape(C, -1)
        g = grad[n].reshape(C, -1)
        for c in range(C):
            ok = a[c] >= 0
            np.add.at(gin[b, c], a[c][ok], g[c][ok])
    return gin.reshape(B, C, H, W).astype(np.float32)
