"""Exact numpy model of the two tables behind the WER / WDER scorer (tal_asrd_amd/wder.py: levenshtein, align_opcodes), swept one
anti-diagonal at a time so that a few hundred thousand cells take milliseconds instead of the seconds of the Python loops:

    D[i][0] = i, D[0][j] = j, D[i][j] = min(D[i-1][j-1] + (a[i-1] != b[j-1]), D[i-1][j] + 1, D[i][j-1] + 1)       (levenshtein)
    M[i][0] = M[0][j] = 0; sm = M[i-1][j-1] + eq, im = M[i][j-1], dm = M[i-1][j]; M[i][j] = max(sm, im, dm)       (align_opcodes)
    back[i][j] = 0 (diagonal) if sm == max, else 1 (insert) if im == max, else 2 (delete); back[i][0] = 2, back[0][j] = 1

The path is read from (m, n) back to (0, 0) and returned in forward order as tag numbers (0 equal, 1 replace, 2 insert, 3 delete:
wder.TAGS); counts[x][y] is the number of equal-or-replace steps whose reference word carries label x and whose hypothesis word
carries label y.  tests/test_edit_ref_cpu.py holds the model to the host routines tuple for tuple."""
import numpy as np

EQUAL, REPLACE, INSERT, DELETE = 0, 1, 2, 3


def tables(a, b):
    """-> (D, back) as (m + 1) x (n + 1) arrays."""
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    m, n = a.size, b.size
    D = np.zeros((m + 1, n + 1), dtype=np.int64)
    M = np.zeros((m + 1, n + 1), dtype=np.int64)
    back = np.zeros((m + 1, n + 1), dtype=np.uint8)
    D[:, 0] = np.arange(m + 1)
    D[0, :] = np.arange(n + 1)
    back[1:, 0] = 2
    back[0, 1:] = 1
    for k in range(2, m + n + 1):
        i = np.arange(max(1, k - n), min(m, k - 1) + 1)
        j = k - i
        eq = (a[i - 1] == b[j - 1]).astype(np.int64)
        D[i, j] = np.minimum(D[i - 1, j - 1] + 1 - eq, np.minimum(D[i - 1, j], D[i, j - 1]) + 1)
        sm, im, dm = M[i - 1, j - 1] + eq, M[i, j - 1], M[i - 1, j]
        mx = np.maximum(sm, np.maximum(im, dm))
        M[i, j] = mx
        back[i, j] = np.where(sm == mx, 0, np.where(im == mx, 1, 2))
    return D, back


def align(a, b, a_labels=None, b_labels=None, n_labels=None):
    """-> (dist, tags uint8 [steps], counts int64 [Ka, Kb] or None)."""
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    D, back = tables(a, b)
    i, j = a.size, b.size
    tags, ii, jj = [], [], []
    while i > 0 or j > 0:
        step = back[i, j]
        if step == 0:
            tags.append(EQUAL if a[i - 1] == b[j - 1] else REPLACE)
            ii.append(i - 1)
            jj.append(j - 1)
            i, j = i - 1, j - 1
        elif step == 1:
            tags.append(INSERT)
            j -= 1
        else:
            tags.append(DELETE)
            i -= 1
    tags = np.array(tags[::-1], dtype=np.uint8)
    counts = None
    if a_labels is not None:
        ka, kb = n_labels if isinstance(n_labels, (tuple, list)) else (n_labels, n_labels)
        counts = np.zeros((ka, kb), dtype=np.int64)
        np.add.at(counts, (np.asarray(a_labels, dtype=np.int64)[np.array(ii, dtype=np.int64)],
                           np.asarray(b_labels, dtype=np.int64)[np.array(jj, dtype=np.int64)]), 1)
    return int(D[a.size, b.size]), tags, counts


def host_counts(ops, a_labels, b_labels, n_labels):
    """The host's matrix: wder.calculate_wder's `sub + cor` label pairs of a list of opcodes, unused labels as zero rows."""
    ka, kb = n_labels if isinstance(n_labels, (tuple, list)) else (n_labels, n_labels)
    counts = np.zeros((ka, kb), dtype=np.int64)
    for t, i0, _, j0, _ in ops:
        if t in ("replace", "equal"):
            counts[a_labels[i0], b_labels[j0]] += 1
    return counts


# ---- seeded contents shared by the CPU and GPU tests
def content(kind, m, n, seed, block_at=None):
    """Two id sequences of lengths m and n.  kind 2 / 3: independent draws from an alphabet of 2 / 3 symbols (ties everywhere: the
    priority rule decides almost every cell); kind 50: b is a copy of a over 50 symbols with about 15 % substitutions and a block of
    a deleted from column `block_at` on (then cut or padded with fresh draws to n)."""
    rng = np.random.default_rng(seed)
    if kind in (2, 3):
        return rng.integers(0, kind, m), rng.integers(0, kind, n)
    a = rng.integers(0, 50, m)
    b = a.copy()
    flip = rng.random(m) < 0.15
    b[flip] = rng.integers(0, 50, int(flip.sum()))
    if block_at is not None and block_at < m:
        b = np.concatenate([b[:block_at], b[block_at + max(1, m // 8):]])
    if b.size < n:
        b = np.concatenate([b, rng.integers(0, 50, n - b.size)])
    return a, b[:n]
