"""Host model of the speaker-turn contract (include/tal_asrd.h, "Speaker turns"): plain NumPy / Python loops, nothing clever.
tests/test_gpu_speaker_turns.py holds every integer output of ops.speaker_turns to exact equality with `speaker_turns` below;
tests/test_turns_ref_cpu.py checks that the model keeps its own contract and that the GPU test's case list (`cases`) tells three
deliberately wrong variants apart.

The three `bug_*` switches exist only for that: each breaks one rule of the contract."""
import numpy as np


class Turns:
    """offsets [B + 1], and per turn start / end (frames relative to the item, end exclusive), label, purity; frame_labels [N]."""

    def __init__(self, offsets, start, end, label, purity, frame_labels):
        self.offsets = np.asarray(offsets, np.int64)
        self.start = np.asarray(start, np.int32)
        self.end = np.asarray(end, np.int32)
        self.label = np.asarray(label, np.int32)
        self.purity = np.asarray(purity, np.int32)
        self.frame_labels = np.asarray(frame_labels, np.int32)


def mode_filter(ids, lo, hi, w, bug_unclipped=False, bug_smallest=False, n_total=None):
    """s[t] for the item ids[lo:hi]: the most frequent id of [t - w, t + w] clipped to the item; among the ids tied for the most,
    ids[t] itself if it is one of them, else the smallest."""
    out = []
    for t in range(lo, hi):
        a, b = max(t - w, lo), min(t + w, hi - 1)
        if bug_unclipped:
            a, b = max(t - w, 0), min(t + w, n_total - 1)
        counts = {}
        for p in range(a, b + 1):
            counts[int(ids[p])] = counts.get(int(ids[p]), 0) + 1
        most = max(counts.values())
        tied = sorted(k for k, v in counts.items() if v == most)
        out.append(int(ids[t]) if int(ids[t]) in tied and not bug_smallest else tied[0])
    return out


def runs_of(s):
    """[(start, end, label)] of the maximal runs of equal values."""
    runs = []
    for t, v in enumerate(s):
        if runs and runs[-1][2] == v:
            runs[-1][1] = t + 1
        else:
            runs.append([t, t + 1, v])
    return runs


def speaker_turns(ids, num_ids, offsets=None, smooth=0, min_frames=1, bug_unclipped=False, bug_prev_item=False, bug_smallest=False):
    ids = np.asarray(ids, np.int64).reshape(-1)
    n = len(ids)
    offsets = [0, n] if offsets is None else [int(x) for x in offsets]
    assert offsets[0] == 0 and offsets[-1] == n and all(a <= b for a, b in zip(offsets, offsets[1:]))
    assert 0 <= smooth <= 31 and min_frames >= 1
    if n and (ids.min() < 0 or ids.max() >= num_ids):
        raise ValueError("an id outside [0, num_ids)")
    turn_off, start, end, label, purity = [0], [], [], [], []
    frame_labels = np.zeros(n, np.int32)
    carry = None      # (bug_prev_item: the last long label of the item before)
    for b in range(len(offsets) - 1):
        lo, hi = offsets[b], offsets[b + 1]
        s = mode_filter(ids, lo, hi, smooth, bug_unclipped, bug_smallest, n)
        runs = runs_of(s)
        is_long = [r[1] - r[0] >= min_frames for r in runs]
        new = [r[2] for r in runs]
        if any(is_long):
            for i in range(len(runs)):
                if is_long[i]:
                    continue
                before = [j for j in range(i) if is_long[j]]
                after = [j for j in range(i + 1, len(runs)) if is_long[j]]
                if before:
                    new[i] = runs[before[-1]][2]
                elif bug_prev_item and carry is not None:
                    new[i] = carry
                else:
                    new[i] = runs[after[0]][2]
            carry = [runs[j][2] for j in range(len(runs)) if is_long[j]][-1]
        merged = []
        for r, lab in zip(runs, new):
            if merged and merged[-1][2] == lab:
                merged[-1][1] = r[1]
            else:
                merged.append([r[0], r[1], lab])
        for a, e, lab in merged:
            start.append(a)
            end.append(e)
            label.append(lab)
            purity.append(int(np.sum(ids[lo + a:lo + e] == lab)))
            frame_labels[lo + a:lo + e] = lab
        turn_off.append(len(start))
    return Turns(turn_off, start, end, label, purity, frame_labels)


def expand(turns, offsets):
    """frame labels rebuilt from the turns"""
    out = np.full(int(offsets[-1]), -1, np.int32)
    for b in range(len(offsets) - 1):
        for k in range(int(turns.offsets[b]), int(turns.offsets[b + 1])):
            out[int(offsets[b]) + int(turns.start[k]):int(offsets[b]) + int(turns.end[k])] = turns.label[k]
    return out


def segment_mean64(feat, ranges):
    """float64 mean of feat[a:b] per range (zeros for an empty one)"""
    feat = np.asarray(feat, np.float64)
    out = np.zeros((len(ranges), feat.shape[1]), np.float64)
    for g, (a, b) in enumerate(ranges):
        if b > a:
            acc = np.zeros(feat.shape[1], np.float64)
            for r in range(int(a), int(b)):
                acc += feat[r]
            out[g] = acc / (b - a)
    return out


def segment_mean_bound(feat, ranges, y64):
    """|y - y64| <= n 2^-24 mean|x| + 2^-24 |y64| per element: the first-order bound of ANY order of n fp32 additions (each of the
    n - 1 partial sums is rounded once, relative 2^-24, and no partial sum exceeds sum|x| = n mean|x| to first order, so the summed
    error is <= (n - 1) 2^-24 sum|x|, i.e. <= n 2^-24 mean|x| after the division by n) plus the rounding of the division."""
    feat = np.asarray(feat, np.float64)
    out = np.zeros_like(y64)
    for g, (a, b) in enumerate(ranges):
        if b > a:
            out[g] = (b - a) * 2.0 ** -24 * np.abs(feat[int(a):int(b)]).mean(axis=0) + 2.0 ** -24 * np.abs(y64[g])
    return out


def sticky_chain(n, labels, stay, seed):
    """random chain: keeps its label with probability `stay`, else draws a new one"""
    rng = np.random.RandomState(seed)
    out = np.zeros(n, np.int32)
    cur = int(rng.randint(labels))
    for t in range(n):
        if rng.rand() > stay:
            cur = int(rng.randint(labels))
        out[t] = cur
    return out


def cases(T, wmax=31):
    """The integer cases of the GPU test: (name, ids, num_ids, offsets | None, smooth, min_frames).  T = the kernels' tile length."""
    out = []
    rng = np.random.RandomState(7)

    def chain(n, labels=3, stay=0.8, seed=None):
        return sticky_chain(n, labels, stay, int(rng.randint(1 << 30)) if seed is None else seed)
    # single-item lengths (w = 5: lengths w and w + 1 as well as 2 w + 1 appear)
    w = 5
    for n in (1, 2, w, w + 1, 2 * w + 1, T - 1, T, T + 1, 2 * T + 1):
        out.append(("len%d" % n, chain(n), 3, None, w, 3))
    for n in (wmax, wmax + 1, 2 * wmax + 1):
        out.append(("len%d_w%d" % (n, wmax), chain(n), 3, None, wmax, 2))
    # ragged batch, empty items in the middle and at the end
    lens = [1, T + 3, 0, 2, T - 1, 0]
    off = np.concatenate([[0], np.cumsum(lens)])
    for w in (0, 1, wmax):
        for m in (1, 2, 50):
            out.append(("ragged_w%d_m%d" % (w, m), chain(int(off[-1]), 3, 0.7), 3, off, w, m))
            out.append(("single_w%d_m%d" % (w, m), chain(T + 77, 4, 0.9), 4, None, w, m))
    # the ends of the id range
    out.append(("id_ends", np.array([0, 6007] * 9 + [6007] * 5 + [0] * 4, np.int32), 6008, None, 2, 2))
    # one turn across tiles; N turns
    out.append(("constant", np.full(4 * T, 5, np.int32), 6, None, 3, 4))
    out.append(("alternating", (np.arange(2 * T + 9) % 2).astype(np.int32), 2, None, 0, 1))
    out.append(("alternating_batch", (np.arange(2 * T + 9) % 2).astype(np.int32), 2, [0, 3, 3, T + 1, 2 * T + 9], 0, 1))
    # hand-written tie windows (w = 1, window of 3 in the middle, of 2 at the ends)
    out.append(("tie2_centre", np.array([4, 2, 2, 7, 7, 1], np.int32), 8, None, 1, 1))        # frame 0: {4, 2} tie, centre 4 stays
    out.append(("tie2_no_centre", np.array([5, 5, 9, 3, 3], np.int32), 10, None, 2, 1))         # frame 2: {5: 2, 3: 2, 9: 1} -> 3
    out.append(("tie3", np.array([8, 6, 7, 1, 1, 1], np.int32), 9, None, 1, 1))                 # frame 1: 8, 6, 7 tie, centre 6 stays
    out.append(("tie3_no_centre", np.array([8, 8, 6, 6, 2, 7, 7, 4, 4], np.int32), 9, None, 4, 1))   # frame 4: 8, 6, 7, 4 tie twice each -> 4
    # step c
    out.append(("short_first_run", np.array([1, 1] + [2] * 6 + [1] + [3] * 5, np.int32), 4, None, 0, 3))
    out.append(("only_short_runs", np.array([1, 1, 2, 2, 3, 1, 1, 0, 5, 5, 5, 5], np.int32), 6, [0, 7, 12], 0, 3))
    out.append(("short_last_then_long_first", np.array([2] * 5 + [1] + [3] * 5 + [0] * 2, np.int32), 4, [0, 6, 13], 0, 3))
    out.append(("short_first_after_long_last", np.array([2] * 5 + [1, 1] + [3] * 5, np.int32), 4, [0, 5, 12], 0, 3))
    out.append(("two_short_in_a_row", np.array([4] * 4 + [1] + [2, 2] + [3] * 4 + [1] + [0], np.int32), 5, None, 0, 3))
    # item boundaries inside a window: w reaches across, the labels differ on the two sides
    out.append(("window_at_boundary", np.array([1, 1, 2, 3, 3, 3, 3, 2, 2, 2], np.int32), 4, [0, 3, 10], 2, 1))
    # random sticky chains
    out.append(("random3", sticky_chain(3 * T + 5, 3, 0.85, 11), 3, None, 6, 13))
    out.append(("random40", sticky_chain(3 * T - 7, 40, 0.6, 12), 40, [0, T - 2, T - 2, 2 * T + 1, 3 * T - 7], 4, 5))
    out.append(("random40_w31", sticky_chain(3 * T + 1, 40, 0.3, 13), 40, [0, 40, T + 9, 3 * T + 1], wmax, 50))
    return out
