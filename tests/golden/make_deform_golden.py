"""Writes tests/golden/deform_reference_cases.npz from the restatement alone (tests/deform_conv_ref.py, form 1):

    python tests/golden/make_deform_golden.py

* `<case>_offset` (int16, units of 2^-10, channels-last) and `<case>_seed` for every row of deform_conv_ref.case_table().
  The offsets are the delicate input and are stored; x, mask, dcols, weight and dy are plain draws that
  deform_conv_ref.case_inputs() repeats from the seed (stored as arrays they would not fit a committed file).
* `T_ref_offset`, `T_ref_mask`, `T_ref_dx`: per tensor max|a - b| / max|b| between form 1 in float32 (sums in the
  reference's order) and form 1 in float64, the maximum over the cases (v1 and v2).

The generator asserts for every case: 10 % .. 50 % of the samples fall outside (-1, H) x (-1, W); at least 5 % of the
coordinates are exact integers; every other coordinate is at least 1e-3 away from an integer.  A seed that misses is
discarded; at most half of the seeds tried may be.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import deform_conv_ref as R     # noqa: E402


def accept(offset, row):
    name, N, C, G, H, W, O, kh, kw, stride, pad, dil = row
    outside, exact, nearest = R.offset_statistics(offset, H, W, G, kh, kw, stride, pad, dil)
    return 0.10 <= outside <= 0.50 and exact >= 0.05 and nearest >= 1e-3, (outside, exact, nearest)


def main():
    out, tried, discarded = {}, 0, 0
    worst = {"T_ref_offset": 0.0, "T_ref_mask": 0.0, "T_ref_dx": 0.0}
    seed = 1000
    for row in R.case_table():
        name, N, C, G, H, W, O, kh, kw, stride, pad, dil = row
        Ho, Wo = R.out_size(H, kh, stride, pad, dil), R.out_size(W, kw, stride, pad, dil)
        while True:
            seed += 1
            tried += 1
            offset = R.make_offsets(np.random.default_rng(seed), N, Ho, Wo, G, kh * kw, span=4, integer_fraction=0.08)
            ok, stats = accept(offset, row)
            if ok:
                break
            discarded += 1
            assert discarded * 2 <= max(tried, 8), "more than half of the seeds discarded (%s: %s)" % (name, stats)
        units = np.round(offset.astype(np.float64) / R.OFFSET_UNIT)
        assert np.array_equal(units * R.OFFSET_UNIT, offset.astype(np.float64)) and np.abs(units).max() < 32768
        out[name + "_offset"], out[name + "_seed"] = units.astype(np.int16), np.int64(seed)
        x, mask, dcols, weight, dy = R.case_inputs(row, seed)
        for m in (None, mask):
            args = (G, kh, kw, stride, pad, dil)
            o32, m32 = R.offset_mask_grad(dcols, x, offset, m, *args, np.float32)
            o64, m64 = R.offset_mask_grad(dcols, x, offset, m, *args, np.float64)
            worst["T_ref_offset"] = max(worst["T_ref_offset"], R.rel_max(o32, o64))
            if m is not None:
                worst["T_ref_mask"] = max(worst["T_ref_mask"], R.rel_max(m32, m64))
            d32 = R.input_grad(dcols, offset, m, x.shape, *args, np.float32)
            d64 = R.input_grad(dcols, offset, m, x.shape, *args, np.float64)
            worst["T_ref_dx"] = max(worst["T_ref_dx"], R.rel_max(d32, d64))
        print(name, "seed", seed, "outside %.3f exact %.3f nearest %.4f" % stats, worst, flush=True)
    assert discarded * 2 <= tried
    out.update({k: np.float64(v) for k, v in worst.items()})
    np.savez_compressed(R.GOLDEN, **out)
    print("tried %d seeds, discarded %d; wrote %s (%d bytes)" % (tried, discarded, R.GOLDEN, os.path.getsize(R.GOLDEN)))


if __name__ == "__main__":
    main()
