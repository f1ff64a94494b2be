"""The numpy model of tests/_edit_ref.py against the host scorer itself (wder.levenshtein / wder.align_opcodes, tuple for tuple), the
rebuild of opcodes from path tags (wder.opcodes_from_tags, with the insert / delete index convention at i = 0 and j = 0), the
word -> id mapping of the device backend, and every `opcodes` entry of tests/golden/wder_unit.json."""
import json
import os

import numpy as np
import pytest

from tal_asrd_amd import wder as W
from tests import _edit_ref as R
from tests.conftest import GOLDEN


def _cases():
    rng = np.random.default_rng(20240611)
    out = []
    for alpha in (2, 3, 50):
        for m, n in ((1, 1), (7, 5), (5, 7), (23, 31), (40, 40), (64, 17)):
            out.append(("random %d %dx%d" % (alpha, m, n), rng.integers(0, alpha, m), rng.integers(0, alpha, n)))
        a = rng.integers(0, alpha, 37)
        out.append(("identical %d" % alpha, a, a.copy()))
        for k in (1, 5):
            out.append(("shifted %d by %d" % (alpha, k), a, np.concatenate([a[k:], rng.integers(0, alpha, k)])))
        out.append(("constant side %d" % alpha, np.zeros(19, dtype=np.int64), rng.integers(0, alpha, 26)))
        out.append(("constant both %d" % alpha, np.zeros(9, dtype=np.int64), np.zeros(14, dtype=np.int64)))
    out.append(("disjoint", rng.integers(0, 5, 21), rng.integers(5, 10, 30)))
    out.append(("disjoint tall", rng.integers(0, 5, 30), rng.integers(5, 10, 21)))
    out.append(("noisy copy", *R.content(50, 48, 44, 3, block_at=16)))
    for m, n in ((0, 0), (0, 1), (1, 0), (0, 9), (9, 0)):
        out.append(("empty %dx%d" % (m, n), rng.integers(0, 3, m), rng.integers(0, 3, n)))
    return out


CASES = _cases()


@pytest.mark.parametrize("name,a,b", CASES, ids=[c[0] for c in CASES])
def test_model_equals_the_host_routines(name, a, b):
    dist, tags, _ = R.align(a, b)
    assert dist == W.levenshtein(a.tolist(), b.tolist())
    ops = W.align_opcodes(a.tolist(), b.tolist())
    assert W.opcodes_from_tags(tags) == ops
    assert [W.TAGS[t] for t in tags] == [o[0] for o in ops]


def test_opcode_rebuild_index_convention_on_the_edges():
    # inserts in front of the first reference word clamp i - 1 to 0, deletes in front of the first hypothesis word clamp j - 1 to 0
    assert W.opcodes_from_tags([2, 2, 0]) == [("insert", 0, 0, 0, 1), ("insert", 0, 0, 1, 2), ("equal", 0, 1, 2, 3)]
    assert W.opcodes_from_tags([3, 3, 1]) == [("delete", 0, 1, 0, 0), ("delete", 1, 2, 0, 0), ("replace", 2, 3, 0, 1)]
    assert W.opcodes_from_tags([0, 2, 3]) == [("equal", 0, 1, 0, 1), ("insert", 0, 0, 1, 2), ("delete", 1, 2, 1, 1)]
    assert W.opcodes_from_tags([]) == []
    assert W.opcodes_from_tags([2]) == W.align_opcodes([], ["x"]) and W.opcodes_from_tags([3]) == W.align_opcodes(["x"], [])
    with pytest.raises(ValueError):
        W.opcodes_from_tags([255])


def test_counts_equal_the_host_matrix():
    rng = np.random.default_rng(5)
    for k in (1, 2, 7):
        a, b = R.content(50, 60, 55, 100 + k, block_at=20)
        la, lb = rng.integers(0, k, a.size), rng.integers(0, k, b.size)
        _, _, counts = R.align(a, b, la, lb, (k + 1, k + 2))
        ops = W.align_opcodes(a.tolist(), b.tolist())
        np.testing.assert_array_equal(counts, R.host_counts(ops, la, lb, (k + 1, k + 2)))
        assert counts.sum() == sum(t in ("equal", "replace") for t, *_ in ops)


def test_word_ids_keep_equality():
    a = ["the", "cat", "the", 7, "7", ("x", 1)]
    b = ["cat", 7, "dog", "the", ("x", 1), "7", "the"]
    ia, ib = W.word_ids(a, b)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            assert (ia[i] == ib[j]) == (x == y)
    for i, x in enumerate(a):
        for j, y in enumerate(a):
            assert (ia[i] == ia[j]) == (x == y)
    assert W.word_ids([], []) == ([], [])


def test_model_reproduces_the_golden_opcodes():
    with open(os.path.join(GOLDEN, "wder_unit.json")) as f:
        unit = json.load(f)
    assert unit["wder"]
    for c in unit["wder"]:
        ia, ib = W.word_ids([w for w, _ in c["ref"]], [w for w, _ in c["hyp"]])
        dist, tags, _ = R.align(ia, ib)
        assert dist == c["dist"]
        assert [list(o) for o in W.opcodes_from_tags(tags)] == c["opcodes"]


def test_backend_argument_is_checked_and_host_stays_the_default():
    ref = [("the", "A"), ("cat", "A"), ("sat", "B")]
    hyp = [("the", 1), ("dog", 1), ("sat", 2)]
    assert W.calculate_wder(ref, hyp)[:4] == W.calculate_wder(ref, hyp, backend="host")[:4] == (1 / 3, 1, 3, 0.0)
    with pytest.raises(ValueError):
        W.calculate_wder(ref, hyp, backend="gpu")
    with pytest.raises(ValueError):
        W.corpus_wder([([("a b", "A")], [("a b", 1)])], backend="cuda")
