"""WER / WDER scoring on the device (csrc/edit_align.hip: tal_edit_align_plan / tal_edit_align_fwd, ops.edit_align, the
backend="device" route of tal_asrd_amd/wder.py) against the exact numpy model of tests/_edit_ref.py and the host routines themselves.
Integers only: every comparison is exact equality.  Shapes sit on the tile edges read back from the library; the raw C-ABI calls
run with guard bytes round every output and a poisoned workspace."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tal_asrd_amd import wder as W
from tests import _edit_ref as R
from tests.conftest import GOLDEN, golden, has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

GUARD = 64            # bytes in front of and behind every output
G_BYTE = 0x5A


def dev():
    return torch.device("cuda:0")


def tile():
    from tal_asrd_amd import ops
    return ops.edit_align_tile()


def _guarded(nbytes):
    return torch.full((GUARD + nbytes + GUARD,), G_BYTE, dtype=torch.uint8, device=dev())


def _unguard(buf, nbytes, what):
    assert bool((buf[:GUARD] == G_BYTE).all()) and bool((buf[GUARD + nbytes:] == G_BYTE).all()), "bytes outside %s written" % what
    return buf[GUARD:GUARD + nbytes].cpu().numpy()


def raw_call(pairs, labels=None, n_labels=None, want_path=True, poison=0xAB):
    """One tal_edit_align_fwd call through the C ABI: guard bytes round stats / path / counts and behind the workspace, the workspace
    filled with `poison` -> (stats [P, 4], [the m + n path bytes of every pair] or None, counts [P, Ka, Kb] or None, launches)."""
    from tal_asrd_amd import _native as N
    lib = N.lib()
    P = len(pairs)
    a_off = np.zeros(P + 1, dtype=np.int64)
    b_off = np.zeros(P + 1, dtype=np.int64)
    np.cumsum([len(a) for a, _ in pairs], out=a_off[1:])
    np.cumsum([len(b) for _, b in pairs], out=b_off[1:])

    def cat(seqs):
        host = np.concatenate([np.asarray(s, dtype=np.int32).reshape(-1) for s in seqs] + [np.zeros(0, dtype=np.int32)])
        return torch.from_numpy(host).to(dev())

    ids_a, ids_b = cat([a for a, _ in pairs]), cat([b for _, b in pairs])
    desc = np.zeros((P, 8), dtype=np.int64)
    nws, npath, nl = C.c_size_t(), C.c_int64(), C.c_int()
    N.check(lib.tal_edit_align_plan(P, a_off.ctypes.data, b_off.ctypes.data, int(want_path), desc.ctypes.data, C.byref(nws), C.byref(npath),
                                    C.byref(nl)), "tal_edit_align_plan")
    assert nws.value == lib.tal_edit_align_workspace_bytes(P, a_off.ctypes.data, b_off.ctypes.data, int(want_path))
    assert npath.value == int(a_off[-1] + b_off[-1])
    desc_dev = torch.from_numpy(desc).to(dev())
    ws = torch.full((nws.value + 256,), poison, dtype=torch.uint8, device=dev())
    stats = _guarded(32 * P)
    path = _guarded(npath.value) if want_path else None
    Ka = Kb = 0
    lab_a = lab_b = counts = None
    if labels is not None:
        Ka, Kb = n_labels
        lab_a, lab_b = cat([x for x, _ in labels]), cat([y for _, y in labels])
        counts = _guarded(8 * P * Ka * Kb)
    N.check(lib.tal_edit_align_fwd(desc.ctypes.data, N.ptr(desc_dev), P, N.ptr(ids_a), N.ptr(ids_b), N.ptr(lab_a), N.ptr(lab_b), Ka, Kb,
                                   C.c_void_p(stats.data_ptr() + GUARD), C.c_void_p(path.data_ptr() + GUARD) if want_path else None,
                                   C.c_void_p(counts.data_ptr() + GUARD) if counts is not None else None, N.ptr(ws), nws.value,
                                   N.stream_handle()), "tal_edit_align_fwd")
    torch.cuda.synchronize()
    assert bool((ws[nws.value:] == poison).all()), "bytes behind the workspace written"
    st = _unguard(stats, 32 * P, "stats").view(np.int64).reshape(P, 4)
    paths = None
    if want_path:
        flat = _unguard(path, npath.value, "path")
        po = a_off + b_off
        paths = [flat[po[p]:po[p + 1]] for p in range(P)]
    cn = None if counts is None else _unguard(counts, 8 * P * Ka * Kb, "counts").view(np.int64).reshape(P, Ka, Kb)
    return st, paths, cn, nl.value


def check_pair(a, b, stats_row, path_bytes, host=False):
    """One pair's outputs against the model (and the host routines): distance, steps, tags, padding, rebuilt opcodes, step counts."""
    dist, tags, _ = R.align(a, b)
    assert int(stats_row[0]) == dist
    assert int(stats_row[1]) == tags.size
    np.testing.assert_array_equal(path_bytes[:tags.size], tags)
    assert bool((path_bytes[tags.size:] == 255).all()) and path_bytes.size == len(a) + len(b)
    assert int(stats_row[2]) == int((tags == R.EQUAL).sum()) and int(stats_row[3]) == int((tags == R.REPLACE).sum())
    ops = W.opcodes_from_tags(path_bytes[:tags.size])
    assert ops == W.opcodes_from_tags(tags)
    if host:
        al, bl = np.asarray(a).tolist(), np.asarray(b).tolist()
        assert dist == W.levenshtein(al, bl)
        assert ops == W.align_opcodes(al, bl)


def ops_call(pairs, **kw):
    """ops.edit_align on a list of pairs -> (stats, the m + n path bytes per pair, counts, result)."""
    from tal_asrd_amd import ops
    res = ops.edit_align([a for a, _ in pairs], [b for _, b in pairs], **kw)
    torch.cuda.synchronize()
    st = res.stats.cpu().numpy()
    paths = None
    if res.path is not None:
        flat = res.path.cpu().numpy()
        paths = [flat[res.path_offsets[p]:res.path_offsets[p + 1]] for p in range(len(pairs))]
    return st, paths, None if res.counts is None else res.counts.cpu().numpy(), res


# ---- 1. shapes on every edge
@pytest.mark.parametrize("kind", [2, 3, 50])
def test_shapes_on_every_tile_edge(kind):
    Rr, Cc = tile()
    ms, ns = (0, 1, Rr - 1, Rr, Rr + 1, 2 * Rr + 1), (0, 1, Cc - 1, Cc, Cc + 1, 2 * Cc + 1)
    shapes = [(m, n) for m in ms for n in ns]
    pairs = [R.content(kind, m, n, 1000 * kind + 37 * i, block_at=Rr) for i, (m, n) in enumerate(shapes)]
    st, paths, _, _ = raw_call(pairs)
    for p, (m, n) in enumerate(shapes):
        check_pair(*pairs[p], st[p], paths[p], host=m <= Rr + 1 and n <= Cc + 1)
    # the distance-only sweep (no second table, no back-pointers)
    st2, none, _, _ = raw_call(pairs, want_path=False)
    assert none is None
    np.testing.assert_array_equal(st2[:, 0], st[:, 0])
    assert not st2[:, 1:].any()


# ---- 2. paths through tile corners
def test_paths_through_tile_corners():
    Rr, Cc = tile()
    rng = np.random.default_rng(77)
    L = Cc + Rr + 7
    a = rng.integers(0, 50, L)
    pairs = [(a, np.concatenate([a[k:], rng.integers(50, 60, k)])) for k in (1, Rr, Cc - 1)]
    pairs += [(np.concatenate([a[k:], rng.integers(50, 60, k)]), a) for k in (1, Rr, Cc - 1)]
    pairs.append((a, a.copy()))                                                      # pure diagonal
    pairs.append((rng.integers(0, 5, Rr + 30), rng.integers(5, 10, Cc + 41)))        # all-zero M: diagonal until an edge, then the boundary rule
    pairs.append((rng.integers(0, 5, Cc + 41), rng.integers(5, 10, Rr + 30)))
    pairs.append((np.zeros(2 * Rr + 2, dtype=np.int64), rng.integers(0, 3, Cc + 44)))   # one side constant
    pairs.append((rng.integers(0, 3, Cc + 44), np.zeros(2 * Rr + 2, dtype=np.int64)))
    st, paths, _, _ = ops_call(pairs)
    for p in range(len(pairs)):
        check_pair(*pairs[p], st[p], paths[p])
    # the shifted paths run beside the diagonal; the identical pair is the diagonal itself
    assert bool((paths[6][:L] == R.EQUAL).all()) and st[6, 0] == 0 and st[6, 1] == L
    assert st[7, 2] == 0 and st[8, 2] == 0


# ---- 3. batch
def _batch_pairs():
    Rr, Cc = tile()
    rng = np.random.default_rng(5)
    shapes = [(0, 5), (1, 1), (2 * Rr + 5, 2 * Cc + 9), (Rr + 6, Cc + 44), (Rr + 6, Cc + 44), (Rr, Cc)]
    pairs = [R.content((2, 3, 50, 3, 50, 2)[i], m, n, 900 + i, block_at=Rr) for i, (m, n) in enumerate(shapes)]
    labels = [(rng.integers(0, 3, m), rng.integers(0, 4, n)) for m, n in shapes]
    return pairs, labels


def test_batch_equals_single_calls_and_repeats_bit_for_bit():
    pairs, labels = _batch_pairs()
    st, paths, cn, launches = raw_call(pairs, labels, (3, 4))
    Rr, Cc = tile()
    assert launches == 3 + 3 - 1 + 1        # the largest pair: 3 x 3 tiles -> 5 anti-diagonals, + the finish kernel
    for p in range(len(pairs)):
        s1, p1, c1, _ = raw_call([pairs[p]], [labels[p]], (3, 4))
        np.testing.assert_array_equal(s1[0], st[p])
        np.testing.assert_array_equal(p1[0], paths[p])
        np.testing.assert_array_equal(c1[0], cn[p])
        check_pair(*pairs[p], st[p], paths[p])
    st2, paths2, cn2, _ = raw_call(pairs, labels, (3, 4))
    assert st2.tobytes() == st.tobytes() and cn2.tobytes() == cn.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(paths, paths2))
    # the wrapper: the same batch in one call, and cut into several by a budget that holds the largest pair only
    kw = dict(a_labels=[x for x, _ in labels], b_labels=[y for _, y in labels], n_labels=(3, 4))
    so, po, co, res = ops_call(pairs, **kw)
    assert res.launches == launches
    sc, pc, cc, res_cut = ops_call(pairs, budget_bytes=max(raw_need(p) for p in pairs), **kw)
    assert res_cut.launches > launches
    for s_, p_, c_ in ((so, po, co), (sc, pc, cc)):
        np.testing.assert_array_equal(s_, st)
        np.testing.assert_array_equal(c_, cn)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(paths, p_))


def raw_need(pair, want_path=True):
    from tal_asrd_amd import _native as N
    oa, ob = np.array([0, len(pair[0])], dtype=np.int64), np.array([0, len(pair[1])], dtype=np.int64)
    return int(N.lib().tal_edit_align_workspace_bytes(1, oa.ctypes.data, ob.ctypes.data, int(want_path)))


# ---- 4. counts
@pytest.mark.parametrize("distinct", [1, 2, 7])
def test_counts_equal_the_host_matrix(distinct):
    Rr, Cc = tile()
    rng = np.random.default_rng(40 + distinct)
    small = R.content(50, 90, 80, 300 + distinct, block_at=30)          # against the host routines
    big = R.content(50, 2 * Rr + 9, 2 * Cc + 3, 400 + distinct, block_at=Rr)      # more than a walk buffer of steps, several tiles
    pairs = [small, big]
    labels = [(rng.integers(0, distinct, len(a)) * 2, rng.integers(0, distinct, len(b)) + 1) for a, b in pairs]
    for n_labels in ((14, 9), (70, 70)):          # counted in LDS / with global atomics (more than 4096 cells)
        st, paths, cn, _ = raw_call(pairs, labels, n_labels)
        ops_small = W.align_opcodes(small[0].tolist(), small[1].tolist())
        np.testing.assert_array_equal(cn[0], R.host_counts(ops_small, labels[0][0], labels[0][1], n_labels))
        for p in range(2):
            _, _, want = R.align(*pairs[p], labels[p][0], labels[p][1], n_labels)
            np.testing.assert_array_equal(cn[p], want)
            assert cn[p].sum() == st[p, 2] + st[p, 3]
            # labels that never occur are zero rows / columns
            assert not cn[p][1::2].any() and not cn[p][:, 0].any() and not cn[p][:, distinct + 1:].any()


def _unit():
    with open(os.path.join(GOLDEN, "wder_unit.json")) as f:
        return json.load(f)


def test_calculate_wder_device_returns_the_host_tuple():
    for c in _unit()["wder"]:
        ref = [tuple(x) for x in c["ref"]]
        hyp = [tuple(x) for x in c["hyp"]]
        assert W.calculate_wer(ref, hyp, backend="device") == (c["wer"], c["dist"], c["n_ref"]) == W.calculate_wer(ref, hyp)
        assert [list(o) for o in W.align_opcodes_device([w for w, _ in ref], [w for w, _ in hyp])] == c["opcodes"]
        wer, dist, n, wder, rl, hl = W.calculate_wder(ref, hyp, backend="device")
        assert (wer, dist, n, wder) == (c["wer"], c["dist"], c["n_ref"], c["wder"])
        assert list(rl) == c["ref_labels"] and list(hl) == c["hyp_labels"]
        h = W.calculate_wder(ref, hyp)
        assert (wer, dist, n, wder) == h[:4] and list(rl) == list(h[4]) and list(hl) == list(h[5])
        assert W.calculate_wder(ref, hyp, wer_only=True, backend="device") == W.calculate_wder(ref, hyp, wer_only=True)


# ---- 5. fixtures
def test_corpus_fixture_on_the_device():
    c = _unit()["corpus"]
    pairs = []
    for r, h in c["pairs"]:
        hyp = [(u, (np.zeros(3), s[1]) if isinstance(s, list) else s) for u, s in h]
        pairs.append(([tuple(x) for x in r], hyp))
    owder, ower, wders, dists, ns = W.corpus_wder(pairs, backend="device")
    assert (owder, ower, dists, ns) == (c["overall_wder"], c["overall_wer"], c["asr_dist"], c["n_words"])
    assert W.corpus_wder(pairs, wer_only=True, backend="device") == W.corpus_wder(pairs, wer_only=True)


def test_episode_fixture_on_the_device():
    """The 1-hour episode's word-level input against the recorded numbers (the host loops are not re-run here)."""
    g = golden("episode_1h")
    with open(os.path.join(GOLDEN, "episode_1h.json")) as f:
        t = json.load(f)
    refs = [(u["utterance"], u["speaker"]) for u in t["ref_utts"]]
    hyps = [(w, (None, int(s))) for w, s in zip(t["word_strs"], g["word_spk"])]
    owder, ower, _, dists, ns = W.corpus_wder([(refs, hyps)], backend="device")
    assert (owder, ower) == (float(g["wder_word"]), float(g["wer_word"]))
    assert dists == g["asr_dist"].tolist() and ns == g["n_words"].tolist()


# ---- 6. guard bands (every raw_call above), workspace contents, errors
def test_result_does_not_depend_on_the_workspace_contents():
    pairs, labels = _batch_pairs()
    base = raw_call(pairs, labels, (3, 4), poison=0xAB)
    for poison in (0x00, 0xFF, 0x55):
        st, paths, cn, _ = raw_call(pairs, labels, (3, 4), poison=poison)
        assert st.tobytes() == base[0].tobytes() and cn.tobytes() == base[2].tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(paths, base[1]))
        st, _, _, _ = raw_call(pairs, want_path=False, poison=poison)
        np.testing.assert_array_equal(st[:, 0], base[0][:, 0])


def _other_launches(fn):
    """Launch scopes of the library's class `other` that `fn` opens (tal_prof_*)."""
    from tal_asrd_amd import _native as N
    lib = N.lib()
    torch.cuda.synchronize()
    N.check(lib.tal_prof_enable(1))
    N.check(lib.tal_prof_reset())
    try:
        fn()
    finally:
        torch.cuda.synchronize()
        ms, n, work = C.c_double(), C.c_int64(), C.c_double()
        N.check(lib.tal_prof_collect(4, C.byref(ms), C.byref(n), C.byref(work)))
        N.check(lib.tal_prof_enable(0))
    return n.value


def test_a_pair_beyond_the_budget_raises_and_launches_nothing():
    from tal_asrd_amd import NativeError, _native as N, ops
    Rr, Cc = tile()
    big = R.content(50, 2 * Rr + 1, 2 * Cc + 1, 1)
    tiny = R.content(3, 5, 7, 2)
    need = raw_need(big)
    assert _other_launches(lambda: ops.edit_align(*tiny)) > 0        # (the counter sees this library's launches)

    def refused():
        with pytest.raises(NativeError) as e:
            ops.edit_align([tiny[0], big[0]], [tiny[1], big[1]], budget_bytes=need - 1)
        msg = str(e.value)
        assert "m=%d" % len(big[0]) in msg and "n=%d" % len(big[1]) in msg and str(need) in msg
    assert _other_launches(refused) == 0
    # the C entry point: a short workspace is TAL_ENOMEM, a descriptor table of the other plan TAL_EINVAL; neither launches
    lib = N.lib()
    a_off, b_off = np.array([0, len(big[0])], dtype=np.int64), np.array([0, len(big[1])], dtype=np.int64)
    desc = np.zeros((1, 8), dtype=np.int64)
    nws = C.c_size_t()
    N.check(lib.tal_edit_align_plan(1, a_off.ctypes.data, b_off.ctypes.data, 1, desc.ctypes.data, C.byref(nws), None, None))
    assert nws.value == need
    ids = torch.zeros(len(big[1]), dtype=torch.int32, device=dev())
    out = torch.zeros(4096, dtype=torch.uint8, device=dev())
    ws = torch.zeros(need, dtype=torch.uint8, device=dev())
    dd = torch.from_numpy(desc).to(dev())

    def short():
        rc = lib.tal_edit_align_fwd(desc.ctypes.data, N.ptr(dd), 1, N.ptr(ids), N.ptr(ids), None, None, 0, 0, N.ptr(out), N.ptr(out), None,
                                    N.ptr(ws), need - 16, N.stream_handle())
        assert rc == -2 and b"workspace" in lib.tal_last_error()
        bad = desc.copy()
        bad[0, 4] = 16
        rc = lib.tal_edit_align_fwd(bad.ctypes.data, N.ptr(dd), 1, N.ptr(ids), N.ptr(ids), None, None, 0, 0, N.ptr(out), N.ptr(out), None,
                                    N.ptr(ws), need, N.stream_handle())
        assert rc == -1 and b"tal_edit_align_plan" in lib.tal_last_error()
    assert _other_launches(short) == 0
    assert not bool(out.any())


def test_strict_raises_on_a_perfect_hypothesis_as_the_host_does():
    ref = [("the", "A"), ("cat", "A"), ("sat", "B"), ("down", "B")]
    hyp = [("the", 7), ("cat", 7), ("sat", 3), ("down", 3)]
    with pytest.raises(ValueError) as host:
        W.calculate_wder(ref, hyp)
    with pytest.raises(ValueError) as device:
        W.calculate_wder(ref, hyp, backend="device")
    assert str(host.value) == str(device.value)
    got = W.calculate_wder(ref, hyp, strict=False, backend="device")
    want = W.calculate_wder(ref, hyp, strict=False)
    assert got[:4] == want[:4] == (0.0, 0, 4, 0.0) and list(got[4]) == list(want[4]) and list(got[5]) == list(want[5])
    # no equal and no replaced word at all: WDER 1.0 without labels
    assert W.calculate_wder([("a", 1)], [], strict=False, backend="device") == W.calculate_wder([("a", 1)], [], strict=False)
    with pytest.raises(ValueError):
        W.corpus_wder([([("a b c", "A")], [("a b c", 1)])], backend="device")
