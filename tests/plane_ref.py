"""The operand-plane definition (csrc/planes.h `split_bf16`, DESIGN.md "Operand planes"), restated in numpy on bit
patterns: uint32 / uint64 integer arithmetic for every rounding, so no library's fp32 -> 16-bit converter is trusted.
The only floating-point operation is the ONE IEEE fp32 subtraction (and, for `transposed`, the one fp32 product) the
definition itself contains.

    bf16x3:  hi = bf16(x),  lo = bf16(fl32(x - hi))          two planes, round-to-nearest-even
    f16:     h  = f16(x * 2^shift)                            one plane; the product is exact (a power of two)
"""
import numpy as np


def _f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


def bits32(x):
    return _f32(x).view(np.uint32)


def widen(h):
    """bf16 words (uint16) -> the fp32 values they are, exactly."""
    return (np.asarray(h, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_rne(x):
    """fp32 -> bf16 word (uint16), round to nearest, ties to even; overflow goes to inf, NaN stays (quiet) NaN."""
    u = bits32(x).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    nan = (u & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    return np.where(nan, ((u >> np.uint64(16)) | np.uint64(0x40)).astype(np.uint16), r)


def split_bf16(x):
    """(hi, lo) words of fp32 x: lo is the bf16 of the fp32-ROUNDED residual x - hi (exact whenever hi is finite)."""
    x = _f32(x)
    hi = bf16_rne(x)
    with np.errstate(invalid="ignore", over="ignore"):
        res = (x - widen(hi)).astype(np.float32)
    return hi, bf16_rne(res)


def split_f16(x, shift=0):
    """fp16 word (uint16) of the exact x * 2^shift, round to nearest even: fp16 subnormals kept, overflow -> inf."""
    u = bits32(x).astype(np.int64)
    sign = ((u >> 31) & 1).astype(np.uint16) << np.uint16(15)
    e = (u >> 23) & 0xFF
    frac = u & 0x7FFFFF
    m = np.where(e > 0, frac | 0x800000, frac)               # |x| = m * 2^(E - 150), E = max(e, 1)
    p = np.maximum(e, 1) - 127 + int(shift)                  # exponent of bit 23 of m, after the shift
    s = np.clip(13 + np.maximum(-14 - p, 0), 13, 40)         # bits of m below one fp16 quantum 2^(max(p, -14) - 10)
    q = m >> s
    rem = m & ((np.int64(1) << s) - 1)
    half = np.int64(1) << (s - 1)
    q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    word = ((np.clip(p, -14, 17) + 14) << 10) + q            # q carries the implicit bit: a carry moves the exponent
    word = np.where((p > 15) | (word >= 0x7C00), 0x7C00, word)
    word = np.where(e == 255, np.where(frac != 0, 0x7E00, 0x7C00), word)
    return word.astype(np.uint16) | sign


def f16_values(h):
    """fp16 words -> fp64, exactly."""
    h = np.asarray(h, dtype=np.uint16).astype(np.int64)
    e, f = (h >> 10) & 0x1F, h & 0x3FF
    mag = np.where(e == 0, np.ldexp(f.astype(np.float64), -24), np.ldexp((f | 0x400).astype(np.float64), e - 25))
    mag = np.where(e == 31, np.where(f != 0, np.nan, np.inf), mag)
    return np.where((h >> 15) == 1, -mag, mag)


def plane_values(hi, lo=None, shift=0):
    """The fp64 value a plane pair (hi + lo) or an fp16 plane (times 2^-shift) stands for."""
    if lo is None:
        return np.ldexp(f16_values(hi), -int(shift))
    with np.errstate(invalid="ignore"):        # (inf + -inf: the pair of an overflowed hi stands for NaN)
        return widen(hi).astype(np.float64) + widen(lo).astype(np.float64)


def paired_index(row, k, K):
    """Word index of hi(row, k) in a PAIRED buffer (csrc/conv_x3.h `x3_paired_index`); its lo word sits 32 words on."""
    return row * 2 * K + (k >> 5) * 64 + (k & 31)


def paired(hi, lo, rows, K):
    """A plane pair [rows][K] (K % 32 == 0) laid out paired: per row, blocks of 32 hi words then their 32 lo words."""
    assert K % 32 == 0
    hi, lo = np.asarray(hi, np.uint16).reshape(rows, K), np.asarray(lo, np.uint16).reshape(rows, K)
    out = np.zeros(2 * rows * K, dtype=np.uint16)
    r, k = np.meshgrid(np.arange(rows), np.arange(K), indexing="ij")
    idx = paired_index(r, k, K)
    out[idx] = hi
    out[idx + 32] = lo
    return out


def transposed(w, row_scale=None):
    """w [O][T][I] fp32 -> the fp32 operand [I][T][O] the transposing split rounds: w * row_scale[o] as ONE fp32
    product (rounded to fp32 BEFORE the split)."""
    w = _f32(w)
    assert w.ndim == 3
    if row_scale is not None:
        w = (w * _f32(row_scale)[:, None, None]).astype(np.float32)
    return np.ascontiguousarray(w.transpose(2, 1, 0))


# ---- the value set every elementwise producer is fed (tests/test_hip_planes.py) -----------------------------------
# (x, hi, lo) worked by hand; inputs whose hi overflows are kept out of `values` (see OVERFLOW)
HAND = [
    (-0.0, 0x8000, 0x0000),
    (1 + 2.0 ** -8, 0x3F80, 0x3B80),                 # tie -> even (down), the residual is the whole 2^-8
    (1 + 2.0 ** -8 + 2.0 ** -23, 0x3F81, 0xBB80),
    (1 + 3 * 2.0 ** -8, 0x3F82, 0xBB80),             # tie -> even (up)
    (3.38e38, 0x7F7E, 0x7A91),
    (65504.0, 0x4780, 0xC200),
    (2.0 ** -126, 0x0080, 0x0000),
    (2.0 ** -133, 0x0001, 0x0000),                   # fp32 subnormal that is an exact bf16 subnormal
    (9.18e-41, 0x0001, 0x8000),                      # just below 2^-133: the residual -3.6e-44 rounds to -0
    (1.4e-45, 0x0000, 0x0000),
]
OVERFLOW = np.array([3.4e38, -3.4e38, 3.3961775e38, -3.3961775e38], dtype=np.float32)   # bf16(x) is +-inf


def values(n, seed=0, f16_shift=None):
    """n finite fp32 values whose hi plane is finite: random mantissas at magnitudes 2^-20 .. 2^20, the hand cases,
    exact bf16 values (lo = 0), ties both ways, +-0, fp32 subnormals, values whose lo is a bf16 subnormal; with
    f16_shift, values around 2^(-24 - shift) (the fp16 plane subnormal) and up to just under 2^(16 - shift) instead of
    the wide magnitudes (every fp16 plane word stays finite)."""
    rng = np.random.default_rng(seed)
    special = [h[0] for h in HAND]
    special += [0.0, -0.0, 1.0, -1.5, 2.0 ** -133, -2.0 ** -149, 3 * 2.0 ** -140, 2.0 ** -127]
    special += [(1 + 2.0 ** -7) * s for s in (1.0, -1.0, 2.0 ** -9, 2.0 ** 11)]                 # exact bf16
    special += [(1 + k * 2.0 ** -8) * s for k in (1, 3, 5, 7) for s in (1.0, -1.0, 2.0 ** -13)]  # ties
    special += [2.0 ** -120 * (1 + 2.0 ** -8 + 2.0 ** -12), -2.0 ** -124 * (1 + 5 * 2.0 ** -9), 2.0 ** -126 * 1.0078]
    if f16_shift is not None:
        lim = 2.0 ** (16 - f16_shift)
        special = [v for v in special if abs(v) < lim * 0.999]
        tiny = 2.0 ** (-24 - f16_shift)
        special += [tiny, -tiny, 0.5 * tiny, 1.5 * tiny, 2.5 * tiny, 0.5000001 * tiny, 1023.5 * tiny, 1024 * tiny,
                    lim * 0.9995, -lim * 0.9995, lim * 0.5, lim * (1 - 2.0 ** -11)]
        mag = np.concatenate([rng.uniform(-26 - f16_shift, 15 - f16_shift, n // 2),
                              rng.uniform(-27 - f16_shift, -12 - f16_shift, n - n // 2)])
    else:
        mag = rng.uniform(-20, 20, n)
    x = (rng.uniform(1, 2, n) * np.exp2(np.floor(mag)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    sp = np.array(special, dtype=np.float32)
    if n >= 8:
        pos = rng.permutation(n)[:min(len(sp), n)]
        x[pos] = sp[:len(pos)]
    else:
        x[:] = sp[rng.permutation(len(sp))[:n]]
    return x
