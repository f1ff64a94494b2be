"""Host side of the resampler (csrc/resample.hip), no GPU: the output-length rule, the filter table the C library builds against the
float64 restatement (tests/_resample_ref.py), the plan limits and argument checks, and properties of the restatement itself."""
import ctypes as C

import numpy as np
import pytest

from tests import _resample_ref as R

PAIRS = [(44100, 16000), (48000, 16000), (8000, 16000), (16000, 8000), (11025, 16000), (16000, 16000), (16001, 16000)]
STANDARD = [(44100, 16000), (48000, 16000), (8000, 16000), (22050, 16000), (11025, 16000), (32000, 16000)]


def _lib():
    from tal_asrd_amd import _native
    return _native.lib()


@pytest.mark.parametrize("orig,new", PAIRS)
def test_output_length(orig, new):
    """tal_resample_num_samples == the restated rule == the count of output instants m / new < L / orig, for every L in 0..2000
    (which includes the exact multiples, where the rule drops one sample)."""
    lib = _lib()
    exact = 0
    for L in range(0, 2001):
        want = R.num_samples(L, orig, new)
        brute = -(-L * new // orig)           # |{m >= 0 : m orig < L new}| = ceil(L new / orig)
        got = lib.tal_resample_num_samples(L, orig, new)
        assert got == want == brute, (L, got, want, brute)
        exact += int(L > 0 and (L * new) % orig == 0)
    assert exact > 0 or R.plan_f64(orig, new)[0] > 2000        # (16001 -> 16000: the first exact multiple is L = 16001)
    assert lib.tal_resample_num_samples((1 << 30) + 12345, 44100, 16000) == R.num_samples((1 << 30) + 12345, 44100, 16000)
    assert lib.tal_resample_num_samples(5, 0, 16000) == 0 and lib.tal_resample_num_samples(-3, 8000, 16000) == 0


def _table(orig, new, width=R.WIDTH):
    lib = _lib()
    taps = C.c_int()
    assert lib.tal_resample_plan_build_host(orig, new, width, None, None, C.byref(taps)) == 0, lib.tal_last_error()
    ou = R.plan_f64(orig, new, width)[1]
    w = np.zeros((ou, taps.value), dtype=np.float32)
    first = np.zeros(ou, dtype=np.int32)
    assert lib.tal_resample_plan_build_host(orig, new, width, w.ctypes.data, first.ctypes.data, C.byref(taps)) == 0
    return taps.value, first, w


@pytest.mark.parametrize("orig,new", PAIRS)
def test_table_matches_the_restatement(orig, new):
    """taps and first[] identical; weights within 1 fp32 ulp of the float64 table (libm and numpy may differ in the last double bit)."""
    iu, ou, taps, first, w = R.plan_f64(orig, new)
    got_taps, got_first, got_w = _table(orig, new)
    assert got_taps == taps
    np.testing.assert_array_equal(got_first.astype(np.int64), first)
    w32 = w.astype(np.float32)
    ulp = np.spacing(np.abs(w32))
    assert np.all(np.abs(got_w.astype(np.float64) - w) <= ulp.astype(np.float64)), float(np.abs(got_w - w32).max())
    assert np.array_equal(got_w == 0, w32 == 0)


def test_prototype_table_shapes():
    for (orig, new), (taps, phases) in {(44100, 16000): (34, 160), (48000, 16000): (37, 1), (8000, 16000): (13, 2),
                                        (22050, 16000): (17, 320), (11025, 16000): (13, 640), (16001, 16000): (13, 16000)}.items():
        _, ou, t, _, _ = R.plan_f64(orig, new)
        assert (t, ou) == (taps, phases), (orig, new, t, ou)


def test_limits():
    lib = _lib()
    for orig, new in PAIRS + STANDARD + [(16000, 44100), (96000, 16000), (192000, 8000)]:
        assert lib.tal_resample_plan_bytes(orig, new, 6) > 0, (orig, new)
    # rates outside 1..2^20, widths outside 1..64, a table beyond 2^20 entries (1048573 and 1048575 are coprime: 2^20 phases x 13
    # taps), a filter beyond 1024 taps (orig / new = 1000)
    for orig, new, width in [(0, 16000, 6), (16000, 0, 6), (-8000, 16000, 6), ((1 << 20) + 1, 16000, 6), (16000, 16000, 0),
                             (16000, 16000, 65), (1048573, 1048575, 6), (1000000, 1000, 6)]:
        assert lib.tal_resample_plan_bytes(orig, new, width) == 0, (orig, new, width)
    taps = C.c_int()
    assert lib.tal_resample_plan_build_host(1048573, 1048575, 6, None, None, C.byref(taps)) == -1
    assert b"2^20" in lib.tal_last_error()
    assert lib.tal_resample_plan_build_host(1000000, 1000, 6, None, None, C.byref(taps)) == -1
    assert b"1024 taps" in lib.tal_last_error()


def test_argument_checks_come_before_any_launch():
    lib = _lib()
    assert lib.tal_resample_fwd(None, 44100, 16000, 6, None, 2, 1, 1000, 1000, None, None, 1000, None) == -1
    assert b"null pointer" in lib.tal_last_error()
    assert lib.tal_resample_fwd(None, 0, 16000, 6, None, 0, 1, 1000, 1000, None, None, 1000, None) == -1
    assert b"sample rates" in lib.tal_last_error()
    assert lib.tal_resample_fwd(None, 44100, 0, 6, None, 0, 1, 1000, 1000, None, None, 1000, None) == -1
    assert lib.tal_resample_fwd(None, 44100, 16000, 6, None, 7, 1, 1000, 1000, None, None, 1000, None) == -1
    assert b"x_dtype" in lib.tal_last_error()
    assert lib.tal_resample_plan_init(None, 44100, 16000, 6, None) == -1


def test_python_surface_without_a_gpu():
    """Resample is a parameter-free module, exported; CPU tensors and int16 without a sample rate are refused by name."""
    import torch
    import tal_asrd_amd as T
    m = T.Resample(44100, 16000)
    assert len(m.state_dict()) == 0 and not list(m.parameters()) and not list(m.buffers())
    assert (m.orig_freq, m.new_freq) == (44100, 16000)
    assert T.ops.resample_num_samples(44100, 44100, 16000) == 16000
    with pytest.raises(T.NativeError):
        m(torch.zeros(1, 4410))
    with pytest.raises(T.NativeError, match="2\\^20"):
        T.Resample(1048573, 1048575)
    sd = T.SDModel()
    keys = list(sd.state_dict())
    with pytest.raises(T.NativeError):
        sd.speaker_ids(torch.zeros(1, 44100, dtype=torch.int16), sample_rate=44100)      # (a CPU tensor)
    assert list(sd.state_dict()) == keys


@pytest.mark.parametrize("orig,new", PAIRS + [(22050, 16000), (32000, 16000), (16000, 44100)])
def test_phase_sums_are_one(orig, new):
    w = R.plan_f64(orig, new)[4]
    s = w.sum(axis=1)
    assert np.all(np.abs(s - 1.0) <= 1e-3), (float(s.min()), float(s.max()))


@pytest.mark.parametrize("orig,new", STANDARD)
def test_a_sine_comes_out_as_that_sine(orig, new):
    """1 kHz, half a second: away from the edges (one filter length either side) the output is the 1 kHz sine at the new rate
    within 2e-3 (measured on the restatement: at most 1.0e-3)."""
    L = orig // 2
    x = np.sin(2 * np.pi * 1000.0 * np.arange(L) / orig)
    y = R.resample_f64(x, orig, new)
    assert y.shape == (R.num_samples(L, orig, new),)
    want = np.sin(2 * np.pi * 1000.0 * np.arange(y.shape[0]) / new)
    edge = 64
    err = float(np.abs(y - want)[edge:-edge].max())
    print("%d -> %d: sine error %.3e" % (orig, new, err))
    assert err <= 2e-3, err


def test_lengths_mean_resample_then_right_pad():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 700))
    y = R.resample_f64(x, 44100, 16000, lengths=[700, 333])
    n1 = R.num_samples(333, 44100, 16000)
    np.testing.assert_array_equal(y[0], R.resample_f64(x[0], 44100, 16000))
    np.testing.assert_array_equal(y[1, :n1], R.resample_f64(x[1, :333], 44100, 16000))
    assert np.all(y[1, n1:] == 0) and n1 < y.shape[1]
    np.testing.assert_array_equal(R.window_f64(x[0, 100:400], 100, 700, 44100, 16000, 60, 40), y[0, 60:100])
