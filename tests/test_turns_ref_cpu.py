"""tests/_turns_ref.py keeps its own contract (the speaker-turn semantics of include/tal_asrd.h), and the case list the GPU test
runs can tell three deliberately wrong variants from the right one.  Also the RTTM text round trip and the constants that
ops.py mirrors from the header.  No GPU."""
import io
import os
import re

import numpy as np
import pytest

from tests import _turns_ref as R
from tests.conftest import ROOT

T = 256      # (the kernels' tile length; the GPU test reads it from the library)


def _rle(ids):
    runs = R.runs_of([int(v) for v in ids])
    return [r[0] for r in runs], [r[1] for r in runs], [r[2] for r in runs]


def test_no_smoothing_is_run_length_encoding():
    for seed in range(4):
        ids = R.sticky_chain(300, 5, 0.7, seed)
        t = R.speaker_turns(ids, 5, None, 0, 1)
        s, e, lab = _rle(ids)
        assert t.start.tolist() == s and t.end.tolist() == e and t.label.tolist() == lab
        assert t.purity.tolist() == [b - a for a, b in zip(s, e)] and int(t.purity.sum()) == len(ids)
        assert t.offsets.tolist() == [0, len(s)]
        np.testing.assert_array_equal(t.frame_labels, ids)


@pytest.mark.parametrize("case", R.cases(T), ids=lambda c: c[0])
def test_contract_on_every_gpu_case(case):
    name, ids, num_ids, off, w, m = case
    n = len(ids)
    off = [0, n] if off is None else [int(x) for x in off]
    t = R.speaker_turns(ids, num_ids, off, w, m)
    # expanding the turns gives frame_labels, and the turns tile every item
    np.testing.assert_array_equal(R.expand(t, off), t.frame_labels)
    assert len(t.offsets) == len(off) and t.offsets[0] == 0 and t.offsets[-1] == len(t.start)
    assert int(t.purity.sum()) <= n and (t.purity >= 0).all()
    if w == 0 and m == 1:
        assert int(t.purity.sum()) == n
    for b in range(len(off) - 1):
        ks = range(int(t.offsets[b]), int(t.offsets[b + 1]))
        length = off[b + 1] - off[b]
        assert (len(ks) == 0) == (length == 0)
        pos = 0
        for k in ks:
            assert t.start[k] == pos and t.end[k] > t.start[k]
            pos = int(t.end[k])
        assert pos == length
        for k0, k1 in zip(ks, ks[1:]):
            assert t.label[k0] != t.label[k1]
        # an item that has a long run: every turn is at least m frames long
        s = R.mode_filter(np.asarray(ids, np.int64), off[b], off[b + 1], w)
        if any(r[1] - r[0] >= m for r in R.runs_of(s)):
            assert all(t.end[k] - t.start[k] >= m for k in ks), name


def test_tie_rule_by_hand():
    f = lambda ids, w: R.mode_filter(np.asarray(ids), 0, len(ids), w)
    assert f([4, 2, 2, 7, 7, 1], 1)[0] == 4            # two-way tie, the centre is in it
    assert f([5, 5, 9, 3, 3], 2)[2] == 3               # two-way tie without the centre: the smallest
    assert f([8, 6, 7, 1, 1, 1], 1)[1] == 6            # three-way tie, the centre is in it
    assert f([8, 8, 6, 6, 2, 7, 7, 4, 4], 4)[4] == 4   # four-way tie without the centre
    assert f([3, 1, 4, 1, 5], 0) == [3, 1, 4, 1, 5]


def test_minimum_duration_by_hand():
    t = R.speaker_turns([1, 1] + [2] * 6 + [1] + [3] * 5, 4, None, 0, 3)
    assert (t.start.tolist(), t.end.tolist(), t.label.tolist(), t.purity.tolist()) == ([0, 9], [9, 14], [2, 3], [6, 5])
    # item 0 has short runs only and keeps them; item 1's short first run looks ahead, never into item 0
    t = R.speaker_turns([1, 1, 2, 2, 3, 1, 1, 0, 5, 5, 5, 5], 6, [0, 7, 12], 0, 3)
    assert t.offsets.tolist() == [0, 4, 5] and t.label.tolist() == [1, 2, 3, 1, 5] and t.end.tolist() == [2, 4, 5, 7, 5]
    # the short last run of item 0 goes to the long run before it, not to item 1's first run
    t = R.speaker_turns([2] * 5 + [1] + [3] * 5 + [0] * 2, 4, [0, 6, 13], 0, 3)
    assert t.label.tolist() == [2, 3] and t.end.tolist() == [6, 7] and t.purity.tolist() == [5, 5]
    # two short runs in a row both go back to the same long run
    t = R.speaker_turns([4] * 4 + [1] + [2, 2] + [3] * 4 + [1] + [0], 5, None, 0, 3)
    assert t.label.tolist() == [4, 3] and t.end.tolist() == [7, 13]


@pytest.mark.parametrize("bug", ["bug_unclipped", "bug_prev_item", "bug_smallest"])
def test_case_list_tells_wrong_variants_apart(bug):
    """a window that is not clipped at the item boundary / a short first run that takes its label from the previous item / ties
    that go to the smallest id even when the centre is among the tied: each differs from the model on at least one GPU case"""
    caught = []
    for name, ids, num_ids, off, w, m in R.cases(T):
        good = R.speaker_turns(ids, num_ids, off, w, m)
        bad = R.speaker_turns(ids, num_ids, off, w, m, **{bug: True})
        same = all(np.array_equal(getattr(good, f), getattr(bad, f)) for f in ("offsets", "start", "end", "label", "purity", "frame_labels"))
        if not same:
            caught.append(name)
    assert caught, bug


def test_bad_ids_raise():
    for bad in (-1, 7):
        with pytest.raises(ValueError):
            R.speaker_turns([0, 1, bad, 2], 7)


def test_segment_mean64_and_bound():
    rng = np.random.RandomState(0)
    x = rng.randn(50, 4).astype(np.float32)
    ranges = [(0, 50), (3, 4), (7, 7), (10, 45)]
    y = R.segment_mean64(x, ranges)
    np.testing.assert_allclose(y[0], x.astype(np.float64).mean(axis=0), rtol=1e-14)
    np.testing.assert_array_equal(y[1], x[3].astype(np.float64))
    assert (y[2] == 0).all()
    # an fp32 left-to-right sum lies inside the bound
    bound = R.segment_mean_bound(x, ranges, y)
    acc = np.zeros(4, np.float32)
    for r in range(10, 45):
        acc = acc + x[r]
    assert (np.abs((acc / np.float32(35)).astype(np.float64) - y[3]) <= bound[3]).all()


def test_rttm_round_trip():
    from tal_asrd_amd import rttm

    class Res:      # what turns_to_seconds reads of a SpeakerTurns result (torch CPU tensors stand in for device ones)
        pass
    import torch
    res = Res()
    res.offsets = torch.tensor([0, 2, 2, 3])
    res.start, res.end = torch.tensor([0, 25, 0], dtype=torch.int32), torch.tensor([25, 40, 100], dtype=torch.int32)
    res.label, res.purity = torch.tensor([7, 6007, 3], dtype=torch.int32), torch.tensor([20, 15, 99], dtype=torch.int32)
    turns = rttm.turns_to_seconds(res, 0)
    assert turns == [(0.0, 25 * 0.08, 7, 20), (25 * 0.08, 40 * 0.08, 6007, 15)]
    assert rttm.turns_to_seconds(res, 1) == []
    assert rttm.turns_to_seconds(res, 2, stride=0.5) == [(0.0, 50.0, 3, 99)]
    fh = io.StringIO()
    assert rttm.write_rttm(fh, "ep1", turns) == 2
    assert fh.getvalue() == ("SPEAKER ep1 1 0.000 2.000 <NA> <NA> 7 <NA> <NA>\n"
                             "SPEAKER ep1 1 2.000 1.200 <NA> <NA> 6007 <NA> <NA>\n")
    back = rttm.read_rttm(io.StringIO(fh.getvalue()))
    assert [(u, lab) for u, _, _, lab in back] == [("ep1", "7"), ("ep1", "6007")]
    for (_, s, e, _), (s0, e0, _, _) in zip(back, turns):
        assert abs(s - s0) < 1e-3 and abs(e - e0) < 1e-3
    with pytest.raises(ValueError):
        rttm.write_rttm(io.StringIO(), "two words", turns)


def test_python_constants_mirror_the_header():
    from tal_asrd_amd import ops
    text = open(os.path.join(ROOT, "include", "tal_asrd.h")).read()
    assert int(re.search(r"#define TAL_TURNS_MAX_HALF (\d+)", text).group(1)) == ops.TURNS_MAX_HALF
    assert int(re.search(r"#define TAL_SEGMENT_MEAN_CHUNK (\d+)", text).group(1)) == ops.SEGMENT_MEAN_CHUNK
    assert ops.speaker_turns_tile() == (T, ops.TURNS_MAX_HALF)
    assert ops.TURNS_MAX_FRAMES == 2 ** 31 - 1 - 2 * T - 2 * ops.TURNS_MAX_HALF


def test_cpu_tensors_raise():
    import torch
    from tal_asrd_amd import NativeError, ops
    with pytest.raises(NativeError):
        ops.speaker_turns(torch.zeros(8, dtype=torch.int32), 4)
    with pytest.raises(NativeError):
        ops.segment_mean(torch.zeros(8, 4), [[0, 8]])
