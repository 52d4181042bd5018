"""The numpy restatement of the operand-plane definition (tests/plane_ref.py) against torch's CPU converters, against
hand-worked words, and against the bounds the definition implies.  Runs anywhere."""
import numpy as np
import pytest
import torch

import plane_ref as P


def _words(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


@pytest.fixture(scope="module")
def wide():
    """2^20 log-uniform magnitudes over e^+-40, both signs, plus the edge list."""
    g = torch.Generator().manual_seed(0)
    mag = torch.exp(torch.rand(1 << 20, generator=g, dtype=torch.float64) * 80 - 40)
    sign = torch.randint(0, 2, (1 << 20,), generator=g) * 2 - 1
    x = torch.cat([(mag * sign).float(), torch.from_numpy(P.values(4096, 1)), torch.from_numpy(P.OVERFLOW)])
    x.requires_grad_(False)
    return x


def test_bf16_split_is_torchs_word_for_word(wide):
    hi, lo = P.split_bf16(wide.numpy())
    th = wide.bfloat16()
    tl = (wide - th.float()).bfloat16()
    assert np.array_equal(hi, _words(th))
    assert np.array_equal(lo, _words(tl))
    assert np.array_equal(P.widen(hi), th.float().numpy())


@pytest.mark.parametrize("shift", [0, 12])
def test_f16_plane_is_torchs_word_for_word(wide, shift):
    edge = torch.tensor([65504.0, 65519.996, 65520.0, -65520.0, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -14,
                         float("inf")]) * 2.0 ** -shift
    x = torch.cat([wide, torch.from_numpy(P.values(4096, 2, f16_shift=shift)), edge])
    h = P.split_f16(x.numpy(), shift)
    assert np.array_equal(h, _words((x.double() * 2.0 ** shift).half()))        # the exact product, rounded once
    assert np.array_equal(P.f16_values(h), torch.from_numpy(h.view(np.int16)).view(torch.float16).double().numpy())
    # overflow to inf starts at 65520 * 2^-shift (shift 12: 15.99609375); the largest finite plane word below it
    assert P.split_f16(np.float32(65520.0 * 2.0 ** -shift).reshape(1), shift)[0] == 0x7C00
    assert P.split_f16(np.float32(65519.996 * 2.0 ** -shift).reshape(1), shift)[0] == 0x7BFF
    # subnormal planes are kept: 2^-24 * 2^-shift is the smallest, half of it ties to even (zero)
    assert P.split_f16(np.float32(2.0 ** (-24 - shift)).reshape(1), shift)[0] == 0x0001
    assert P.split_f16(np.float32(-2.0 ** (-25 - shift)).reshape(1), shift)[0] == 0x8000


def test_hand_cases():
    for x, hi, lo in P.HAND:
        h, l = P.split_bf16(np.array([x], dtype=np.float32))
        assert (int(h[0]), int(l[0])) == (hi, lo), (x, hex(h[0]), hex(l[0]))
    # hi overflows: finite - inf is the other infinity, and the pair stands for NaN
    h, l = P.split_bf16(P.OVERFLOW)
    assert list(h) == [0x7F80, 0xFF80, 0x7F80, 0xFF80] and list(l) == [0xFF80, 0x7F80, 0xFF80, 0x7F80]
    assert np.isnan(P.plane_values(h, l)).all()
    assert P.bf16_rne(np.array([np.nan], dtype=np.float32))[0] & 0x7FC0 == 0x7FC0


def test_reconstruction_bound(wide):
    """Two roundings to 8 significant bits: |hi + lo - x| <= 2^-17 |x| (where lo is a normal bf16: |x| >= 2^-100 is
    ample)."""
    x = wide.numpy()
    hi, lo = P.split_bf16(x)
    ok = np.isfinite(P.widen(hi)) & (np.abs(x) >= 2.0 ** -100)
    assert ok.sum() > 1 << 19
    v = P.plane_values(hi, lo)[ok]
    xd = x[ok].astype(np.float64)
    assert (np.abs(v - xd) <= 2.0 ** -17 * np.abs(xd)).all()
    # the fp16 plane: one rounding to 11 bits in the normal range
    xs = P.values(1 << 16, 3, f16_shift=12)
    h = P.split_f16(xs, 12)
    normal = np.abs(xs) >= 2.0 ** (-14 - 12)
    err = np.abs(P.plane_values(h, None, 12) - xs.astype(np.float64))
    assert (err[normal] <= 2.0 ** -11 * np.abs(xs[normal])).all()
    assert (err[~normal] <= 2.0 ** (-25 - 12)).all()


@pytest.mark.parametrize("K", [32, 64, 288])
def test_paired_index_is_a_bijection_onto_the_hi_slots(K):
    rows = 5
    r, k = np.meshgrid(np.arange(rows), np.arange(K), indexing="ij")
    idx = P.paired_index(r, k, K).reshape(-1)
    every = np.arange(2 * rows * K)
    hi_slots = every[(every % 64) < 32]
    assert np.array_equal(np.sort(idx), hi_slots)
    assert np.array_equal(np.sort(np.concatenate([idx, idx + 32])), every)
    hi = np.arange(rows * K, dtype=np.uint16)
    lo = hi + np.uint16(30000)
    buf = P.paired(hi, lo, rows, K).reshape(rows, K // 32, 2, 32)       # the layout in words: [row][block][hi|lo][32]
    assert np.array_equal(buf[:, :, 0].reshape(-1), hi) and np.array_equal(buf[:, :, 1].reshape(-1), lo)


def test_transposed_round_trips_against_a_plain_permute():
    g = torch.Generator().manual_seed(4)
    w = torch.randn(7, 3, 5, generator=g)
    s = torch.rand(7, generator=g) + 0.5
    assert np.array_equal(P.transposed(w.numpy()), w.permute(2, 1, 0).contiguous().numpy())
    assert np.array_equal(P.transposed(P.transposed(w.numpy())), w.numpy())
    assert np.array_equal(P.transposed(w.numpy(), s.numpy()), (w * s.view(-1, 1, 1)).permute(2, 1, 0).contiguous().numpy())
    # the product is rounded to fp32 before the split: the residual of the EXACT product differs on some words
    wt = P.transposed(w.numpy(), s.numpy())
    hi, lo = P.split_bf16(wt)
    exact = w.double().numpy().transpose(2, 1, 0) * s.double().numpy()[None, None, :]
    assert np.abs(P.plane_values(hi, lo) - wt.astype(np.float64)).max() <= 2.0 ** -17 * np.abs(wt).max()
    assert np.abs(wt.astype(np.float64) - exact).max() > 0


def test_value_set_holds_what_it_promises():
    x = P.values(2048, 0)
    hi, lo = P.split_bf16(x)
    assert np.isfinite(x).all() and np.isfinite(P.widen(hi)).all()
    u = P.bits32(x)
    assert ((u & 0x7F800000) == 0).sum() >= 4 and (u == 0x80000000).any() and (u == 0).any()      # subnormals, +-0
    assert ((lo & 0x7FFF) == 0).sum() >= 8                                                       # exact bf16 values
    assert (((lo & 0x7F80) == 0) & ((lo & 0x7F) != 0)).any()                                     # lo a bf16 subnormal
    assert ((u & 0xFFFF) == 0x8000).sum() >= 8                                                   # ties
    for shift in (0, 12):
        h = P.split_f16(P.values(2048, 0, f16_shift=shift), shift)
        assert ((h & 0x7C00) != 0x7C00).all()
        assert (((h & 0x7C00) == 0) & ((h & 0x3FF) != 0)).sum() > 100
        assert (h & 0x7FFF).max() >= 0x7BF0
