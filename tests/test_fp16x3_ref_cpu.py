"""The NumPy restatement of the fp16x3 format (tests/_fp16x3_ref.py) tied down on the CPU, the seeded head inputs checked
against the skip condition of the GPU head tests, and the site table of tests/test_gpu_fp16x3_range.py checked against the
sources."""
import glob
import os
import re

import numpy as np

from tests import _fp16x3_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _all_f16():
    h = np.arange(0, 1 << 16, dtype=np.uint16).view(np.float16)
    return h[np.isfinite(h)]


def test_round_trip_is_exact_for_every_fp16_value():
    h = _all_f16()
    for split in (R.split_clamped, R.split_plain):
        hi, lo = split(h.astype(np.float32))
        assert np.array_equal(hi.view(np.uint16), h.view(np.uint16))
        assert not lo.astype(np.float32).any()
        assert np.array_equal(R.decode(hi, lo), h.astype(np.float64))


def test_normal_range_keeps_22_bits():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(200000) * 2.0 ** rng.integers(-13, 15, 200000)).astype(np.float32)
    x = x[(np.abs(x) >= R.F16_MIN_NORMAL * 2) & (np.abs(x) <= R.F16_MAX)]
    for split in (R.split_clamped, R.split_plain):
        d = R.decode(*split(x))
        assert np.all(np.abs(d - x.astype(np.float64)) <= 2.0 ** -22 * np.abs(x))


def test_below_the_normal_range_the_documented_bound_holds():
    """hi is a multiple of 2^-24 (fp16 subnormal grid), lo a multiple of 2^-24 scaled by 2^-11: the carried value is within
    2^-36 of x everywhere below 2^-14, so a product with w errs by at most 2^-35 |w| -- the header's figure."""
    rng = np.random.default_rng(1)
    x = (rng.uniform(-1, 1, 200000) * 2.0 ** rng.integers(-45, -13, 200000)).astype(np.float32)
    x = np.concatenate([x, R.interesting_f32_patterns()])
    x = x[np.abs(x) < R.F16_MIN_NORMAL]
    d = R.decode(*R.split_clamped(x))
    assert np.all(np.abs(d - x.astype(np.float64)) <= 2.0 ** -36)
    tiny = x[np.abs(x) < 2.0 ** -25]
    assert not R.split_clamped(tiny)[0].astype(np.float32).any()          # below half the smallest subnormal hi is zero ...
    assert np.all(np.abs(R.decode(*R.split_clamped(tiny)) - tiny) <= 2.0 ** -36)   # ... and lo alone carries the value


def test_subnormal_halves_are_kept():
    x = np.float32(2.0 ** -20 * 1.25)
    hi, lo = R.split_clamped(x)
    assert float(hi) == 2.0 ** -20 * 1.25 and float(lo) == 0.0
    x = np.float32(2.0 ** -24 * 1.5)
    hi, lo = R.split_clamped(x)
    assert float(hi) == 2.0 ** -23 and float(lo) == -(2.0 ** -25) * 2048


def test_clamping_is_monotone_above_the_range():
    x = np.concatenate([np.arange(65000, 66000, 0.25), np.geomspace(66000, 3e38, 2000)]).astype(np.float32)
    d = R.decode(*R.split_clamped(x))
    assert np.all(np.diff(d) >= 0) and d.max() == 65504.0 + 65504.0 / 2048.0
    d = R.decode(*R.split_clamped(-x))
    assert np.all(np.diff(d) <= 0) and d.min() == -(65504.0 + 65504.0 / 2048.0)
    inside = x <= 65504.0 + 31.0                                          # the low half still carries up to 65504 / 2048 ~ 32 beyond the top
    assert np.array_equal(R.decode(*R.split_clamped(x[inside])), x[inside].astype(np.float64))


def test_nonfinite_table():
    def same(got, want):
        return np.isnan(got) if isinstance(want, str) else float(got) == want
    for x, (ch, cl), (ph, pl), guard in R.NONFINITE_TABLE:
        hi, lo = R.split_clamped(np.float32(x))
        assert same(hi, ch) and same(lo, cl), (x, hi, lo)
        hi, lo = R.split_plain(np.float32(x))
        assert same(hi, ph) and same(lo, pl), (x, hi, lo)
        assert bool(R.out_of_range(x)) == guard, x
        # the contract of the guarded kernels: out of range -> the flag; and the plain halves of a non-finite value are not finite
        if not np.isfinite(x):
            assert not np.isfinite(R.decode(hi, lo))


def test_byte_geometry_round_trip():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((5, 96)).astype(np.float32)
    hi, lo = R.split_clamped(x)
    words = R.pack_rows(hi, lo)
    assert words.shape == (5, 3, 64) and words.nbytes == x.nbytes
    assert np.array_equal(words[2, 1, :32], hi[2, 32:64].view(np.uint16)) and np.array_equal(words[2, 1, 32:], lo[2, 32:64].view(np.uint16))
    h2, l2 = R.unpack_rows(words.reshape(-1), 5, 96)
    assert np.array_equal(h2, hi) and np.array_equal(l2, lo)


def test_product_matches_float64_to_the_dropped_term():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((40, 256)).astype(np.float32)
    w = rng.standard_normal((24, 256)).astype(np.float32)
    want = x.astype(np.float64) @ w.astype(np.float64).T
    got = R.product_f16x3(x, w)
    bound = 3 * 2.0 ** -22 * (np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64).T)   # two operand roundings + lo * lo
    assert np.all(np.abs(got - want) <= bound)


def test_head_inputs_meet_the_skip_condition():
    """float64 reference alone: on the seeded head inputs at most 1 % of the rows have a top-2 margin within 8 * e32."""
    for p in R.SWEEP_EXPONENTS:
        feat, wl, bl = R.head_case(p)
        _, _, keep, e32 = R.head_reference(feat, wl, bl)
        assert (~keep).mean() <= 0.01, (p, float((~keep).mean()), e32)


# ---------------------------------------------------------------------------------------------------------------------
CALLS = {"note_range": r"\bnote_range\(", "split_f16x3": r"\bsplit_f16x3\(", "split_f16x3_pair": r"\bsplit_f16x3_pair\("}
FUNC = re.compile(r"^(?![#/\s}])[^;]*\b(?:void|int|bool|size_t|float|int64_t)\s+(\w+)\s*\([^;]*$")


def _scan_sources():
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tal_asrd_amd", "csrc", "*"))):
        cur = None
        for line in open(path):
            m = FUNC.match(line)
            if m:
                cur = m.group(1)
                if cur in CALLS:
                    continue                                   # the definitions themselves (common.h)
            code = line.split("//")[0]
            for name, pat in CALLS.items():
                n = len(re.findall(pat, code))
                if n:
                    d = found.setdefault((os.path.basename(path), cur), {})
                    d[name] = d.get(name, 0) + n
    return found


def test_site_table_accounts_for_every_converting_call():
    """every note_range / split_f16x3 / split_f16x3_pair call in the sources belongs to a row of the GPU file's site table, with
    the same counts: a new converting site fails here until the table names it (and says which case covers it)."""
    from tests.test_gpu_fp16x3_range import SITES
    table = {(f, fn): calls for f, fn, calls, _, _, _ in SITES}
    assert len(table) == len(SITES)
    found = _scan_sources()
    assert found == table, {"only in the sources": {k: v for k, v in found.items() if table.get(k) != v},
                            "only in the table": {k: v for k, v in table.items() if found.get(k) != v}}
    for _, _, _, guard, reach, test in SITES:
        assert guard and reach and test
