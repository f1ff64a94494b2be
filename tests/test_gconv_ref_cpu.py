"""tests/_gconv_ref.py without a GPU: the float64 model equals its three-loop restatement, the exactness premises hold on the data
of every case of the table, `check` accepts the model's own answer in banded buffers and rejects every mutant on a case of the
table (the witness is named beside each mutant)."""
import numpy as np
import pytest

from tests import _gconv_ref as R

KEYS = sorted({c.key for c in R.CASES})
# one case per (entry, problem): the options change which kernel runs, not what it has to return
PROBLEMS = sorted({(c.entry, c.key): c for c in R.CASES}.values(), key=lambda c: (c.key, c.entry))


def _case(entry, stride, cig, cog, G, k, B, T):
    hits = [c for c in R.CASES if c.entry == entry and c.key == R.Key(stride, cig, cog, G, k, B, T)]
    assert hits, "not in the table: %s %s" % (entry, (stride, cig, cog, G, k, B, T))
    return hits[0]


@pytest.mark.parametrize("stride,cig,cog,G,k,B,T", [
    (1, 10, 10, 2, 21, 2, 13), (1, 18, 18, 2, 21, 1, 1), (1, 4, 4, 2, 3, 2, 5), (1, 3, 3, 1, 63, 1, 40), (1, 2, 2, 3, 1, 2, 4),
    (2, 1, 10, 4, 21, 2, 24), (2, 10, 14, 2, 21, 1, 21), (2, 14, 18, 2, 21, 2, 26), (2, 2, 3, 2, 8, 2, 13), (2, 2, 3, 2, 1, 1, 6)])
def test_reference_equals_the_loops(stride, cig, cog, G, k, B, T):
    key = R.Key(stride, cig, cog, G, k, B, T)
    w, b = R.weights(stride, cig, cog, G, k)
    x = R.x_of(key)
    want = R.reference_loops(x, w, b, stride, G)
    np.testing.assert_array_equal(R.reference(x, w, b, stride, G), want)
    np.testing.assert_array_equal(R.wrong_model(key), want)            # the mutants' generator with no rule broken


def test_pack_weight_is_the_library_layout():
    """dst[((g * cig + ci) * k + j) * cog + co] = src[((g * cog + co) * cig + ci) * k + j] (pack_gconv_kernel)."""
    G, cog, cig, k = 3, 5, 2, 4
    w = np.arange(G * cog * cig * k, dtype=np.float64).reshape(G * cog, cig, k)
    p = R.pack_weight(w, G).reshape(-1)
    for i in range(p.size):
        co, t = i % cog, i // cog
        j, t = t % k, t // k
        ci, g = t % cig, t // cig
        assert p[i] == w[g * cog + co, ci, j]


def test_split_form_round_trip_and_layout():
    v = np.asarray([[1.0 + 2.0 ** -15, -3.5, 12111.9375, 0.0] * 16], dtype=np.float64)
    u = R.encode_split(v)
    assert u.shape == (1, 2, 64)
    np.testing.assert_array_equal(R.decode_split(u, 1, 64), v)
    h = u.view(np.float16)
    assert h[0, 0, 0] == 1.0 and h[0, 0, 32] == np.float16(2.0 ** -4) and h[0, 1, 1] == -3.5 and h[0, 1, 33] == 0.0


def test_exactness_premises_hold_for_every_problem_of_the_table():
    lo_share = {}
    for key in KEYS:
        w, b = R.weights(key.stride, key.cig, key.cog, key.G, key.k)
        x = R.x_of(key)
        assert np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 8 and np.array_equal(w, np.rint(w)) and np.abs(w).max() <= 4, key
        assert np.abs(b).max() <= 16 and np.array_equal(b * 16, np.rint(b * 16)), key
        if key.stride == 1:
            assert np.array_equal(b, np.rint(b)), key
        # every operand is one fp16 half
        assert np.array_equal(x.astype(np.float16).astype(np.float32), x) and np.array_equal(w.astype(np.float16).astype(np.float64), w), key
        # any partial sum, in any order, stays below sum |x| |w| + |b| <= 8 * sum |w| + 16 < 2^20 with at most 4 fractional bits
        bound = 8.0 * np.abs(w).sum(axis=(1, 2)).max() + 16.0
        assert bound < 2.0 ** 20 and bound <= 8 * 4 * key.cig * key.k + 16, key
        m = R.model(key)
        assert np.isfinite(m).all() and np.array_equal(m.astype(np.float32).astype(np.float64), m), key
        C = key.G * key.cog
        if C % 32 == 0 and key.k == 21:
            u = R.encode_split(m.reshape(-1, C))
            assert np.array_equal(R.decode_split(u, m.size // C, C), m.reshape(-1, C)), key
            lo = u.reshape(-1, C // 32, 2, 32)[:, :, 1]
            lo_share.setdefault((key.stride, key.cig), []).append(float(np.mean((lo & 0x7FFF) != 0)))
    # the lo halves of the outputs are busy: a kernel that drops them is seen (the 1 -> 10 conv: 21 products only)
    for (stride, cig), shares in lo_share.items():
        assert np.mean(shares) > (0.2 if cig > 1 else 0.01), (stride, cig, np.mean(shares))


def test_check_accepts_the_models_own_answer():
    for case in PROBLEMS:
        R.check(case, R.perfect_outputs(case))


def test_check_takes_minus_zero_for_zero():
    case = _case("res", 1, 10, 10, 16, 21, 1, 16)
    m = R.model(case.key).copy()
    assert (m == 0).any()
    m[m == 0] = -0.0
    R.check(case, R.perfect_outputs(case, m))


def test_banded_inputs():
    x = R.x_of(R.Key(1, 10, 10, 16, 21, 2, 9))
    for split in (False, True):
        buf, off = R.banded_input(x, split)
        row = 160 * 4
        assert off == R.FRONT * row and off % 16 == 0 and buf.size == (R.FRONT + 18 + R.BACK) * row
        bands = np.concatenate([buf[:off], buf[off + 18 * row:]])
        if split:
            assert np.isnan(bands.view(np.float16)).all()
            np.testing.assert_array_equal(R.decode_split(buf[off:off + 18 * row].view(np.uint16), 18, 160), x.reshape(18, 160))
        else:
            assert np.isnan(bands.view(np.float32)).all()
            np.testing.assert_array_equal(buf[off:off + 18 * row].view(np.float32), x.reshape(-1))
    for halves, dt in ((False, np.float32), (True, np.float16)):
        b = R.with_nan_band(np.arange(7, dtype=np.float32), halves)
        assert b.size == 32 + R.AUX_BAND and np.array_equal(b[:28].view(np.float32), np.arange(7)) and np.isnan(b[32:].view(dt)).all()


# mutant -> the witness: a case of the table on which check() must fail
WITNESS = {
    "back_band_written": ("res_split", 1, 18, 18, 16, 21, 2, 17),
    "back_band_written_far": ("s2_k", 2, 1, 10, 20, 8, 2, 40),
    "front_band_written": ("s2_f16x3", 2, 10, 14, 16, 21, 1, 21),
    "last_row_not_stored": ("res_f16x3_ys", 1, 14, 14, 16, 21, 2, 257),
    "first_row_of_item_1_not_stored": ("s2_split", 2, 10, 14, 16, 21, 2, 53),
    "taps_reversed": ("res", 1, 10, 10, 16, 21, 1, 2),                       # (T = 1 would not do: the middle tap is its own mirror image)
    "padding_9": ("res_f16x3", 1, 10, 10, 16, 21, 1, 2),
    "padding_11": ("res_k", 1, 4, 4, 8, 3, 2, 2),
    "no_padding_between_items": ("res_split", 1, 18, 18, 16, 21, 2, 1),
    "s2_windows_start_at_2t_plus_1": ("s2", 2, 1, 10, 80, 21, 64, 21),
    "s2_odd_last_row_is_a_window": ("s2_split_f32in", 2, 14, 18, 16, 21, 1, 22),
    "relu_missing": ("res_k", 1, 10, 10, 3, 1, 2, 1),
    "residual_from_row_t_minus_1": ("res", 1, 18, 18, 16, 21, 2, 2),
    "residual_from_row_t_plus_1": ("res_f16x3", 1, 18, 18, 12, 21, 2, 17),
    "split_lo_zeroed": ("s2_split", 2, 10, 14, 16, 21, 1, 21),
    "split_hi_lo_swapped_in_one_block": ("res_f16x3_ys", 1, 10, 10, 16, 21, 1, 1),
    "channels_16_17_exchanged": ("res_split", 1, 18, 18, 16, 21, 1, 1),
    "conv_over_the_poisoned_buffer": ("res_f16x3", 1, 14, 14, 16, 21, 1, 300),
}


def test_every_mutant_has_a_witness():
    assert set(WITNESS) == set(R.MUTANTS)


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_check_rejects_the_mutant(mutant):
    case = _case(*WITNESS[mutant])
    bufs = R.MUTANTS[mutant](case)
    assert bufs is not None, "the mutant does not apply to its witness"
    with pytest.raises(AssertionError, match=case.name.replace("+", r"\+")):
        R.check(case, bufs)


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
def test_mutants_are_rejected_on_every_problem_they_change(mutant):
    """Over a slice of the table (every 19th problem): wherever the mutant's buffers differ from the perfect ones, check() fails; where
    they do not, it passes.  check() has no blind spot that depends on the shape."""
    hits = 0
    for case in PROBLEMS[::19]:
        if case.key.B > 2 or case.key.G > 16:
            continue
        bufs = R.MUTANTS[mutant](case)
        if bufs is None:
            continue
        same = all(np.array_equal(a, b) for a, b in zip(bufs, R.perfect_outputs(case)))
        if same:
            R.check(case, bufs)
            continue
        hits += 1
        with pytest.raises(AssertionError):
            R.check(case, bufs)
    assert hits > 0, mutant


def test_the_table_covers_what_the_issue_names():
    by_entry = {}
    for c in R.CASES:
        by_entry.setdefault(c.entry, []).append(c)
    assert set(by_entry) == set(R.ENTRIES)
    for entry in ("res", "res_f16x3", "res_f16x3_ys", "res_split"):
        for cg in (10, 14, 18):
            ts = {(c.key.T, c.key.B) for c in by_entry[entry] if c.key.cig == cg and c.key.G == 16}
            assert ts == {(T, B) for T in R.T_S1 for B in (1, 2)}, (entry, cg)
    for entry in ("s2", "s2_f16x3", "s2_split", "s2_split_f32in"):
        for cig in (10, 14):
            ts = {(c.key.T, c.key.B) for c in by_entry[entry] if c.key.cig == cig and c.key.G == 16}
            assert ts == {(2 * to + 19 + odd, B) for to in R.TOUT_S2 for odd in (0, 1) for B in (1, 2)}, (entry, cig)
    for entry in R.MFMA_ENTRIES:
        opts = [dict(c.opts) for c in by_entry[entry]]
        assert {o["gconv_short_below"] for o in opts} == {0, 1 << 20} and {o["gconv_long_tt"] for o in opts} == {0, 128, 256}
        assert {o["gconv_grid_xyz"] for o in opts} == {0, 1}
        assert {c.key.G for c in by_entry[entry]} >= ({16, 80, 64} if "split" in entry or entry == "res_f16x3_ys" else {16, 80, 40, 64})
    assert {dict(c.opts)["gconv_no_shift18"] for c in by_entry["res_split"] if c.key.cig == 18} == {0, 1}
    assert any(c.key.G == 12 and c.key.cig == 18 for c in by_entry["res_f16x3"])
    assert {c.key.k for c in by_entry["res_k"]} == {1, 3, 15, 21, 31, 63} and {c.key.k for c in by_entry["s2_k"]} == {1, 3, 8, 15, 21, 31, 63}
    assert {(c.key.B, c.key.T) for c in by_entry["s2"] if c.key.cig == 1 and c.key.G == 80} >= {(64, 21), (64, 85), (64, 600), (1, 600)}
    assert any(dict(c.opts).get("gconv_c1_generic") == 1 for c in by_entry["s2"])
    # options are the library's names and every case spells out the ones it depends on
    for c in R.CASES:
        assert set(dict(c.opts)) <= set(R.OPTION_DEFAULTS), c.name
