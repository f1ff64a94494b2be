"""The attention pooling and the speaker votes written out from the reference's statements, in plain Python and numpy.

tal/utils/aligned_to_wder_format.py:150-214 (per word: a dict of summed attention per speaker id, the word's embeddings;
per utterance: the embeddings) and :321-353 (aligned: Counter(ids[st:e]).most_common(1)).  Nothing here calls the library:
tests compare the kernels of csrc/pool.hip with it (tests/test_gpu_pool_kernels.py), and tests/test_pool_ref_cpu.py compares
it with what the reference itself produced (tests/golden/pool_unit.*, aligned_unit.*).

Every rule the kernels have to get right is a field of `Rules`; KNOBS lists, per rule, the plausible wrong variants.  CASES is
the table of inputs the GPU test runs; `outputs(case, mode, rules)` is what a perfect kernel under `rules` returns and
`compare(case, mode, got)` the comparison the GPU test applies.  A case tests a rule only if compare() rejects the outputs of
the wrong variant -- tests/test_pool_ref_cpu.py asserts that for every knob."""
from collections import Counter, namedtuple
from functools import lru_cache

import numpy as np

INF = float("inf")
U32, U64 = 2.0 ** -24, 2.0 ** -53          # unit roundoff of fp32 / float64

# tie_*: which of the ids with the largest weight wins -- "first" / "last" to appear (insertion order of the dict) or the "lowest"
# id.  wrap_negative: negative starts count from the end (python slices) instead of being clamped to 0.  truncate: attention is
# cut to the window length, aw[:len(chunk)]; the wrong variant keeps all S entries and pairs those past the window with its last
# frame (an index clamp).  round_fp16: half mode rounds attention (and features) to fp16 first.  ignore_out_of_range: ids
# outside [0, num_ids) do not vote in the two group kernels.
Rules = namedtuple("Rules", "tie_vote tie_groups tie_major wrap_negative truncate round_fp16 ignore_out_of_range")
RULES = Rules("first", "last", "first", True, True, True, True)
KNOBS = {
    "vote_tie_last": RULES._replace(tie_vote="last"),
    "vote_tie_lowest": RULES._replace(tie_vote="lowest"),
    "groups_tie_first": RULES._replace(tie_groups="first"),
    "groups_tie_lowest": RULES._replace(tie_groups="lowest"),
    "major_tie_last": RULES._replace(tie_major="last"),
    "major_tie_lowest": RULES._replace(tie_major="lowest"),
    "clamp_negative": RULES._replace(wrap_negative=False),
    "no_truncation": RULES._replace(truncate=False),
    "no_fp16": RULES._replace(round_fp16=False),
    "count_out_of_range": RULES._replace(ignore_out_of_range=False),
}
# the knobs that can change a kernel of each kind
KNOBS_OF = {"vote": ("vote_tie_last", "vote_tie_lowest", "clamp_negative", "no_truncation"),
            "groups": ("groups_tie_first", "groups_tie_lowest", "clamp_negative", "no_truncation", "no_fp16", "count_out_of_range"),
            "major": ("major_tie_last", "major_tie_lowest", "clamp_negative", "count_out_of_range"),
            "pool": ("clamp_negative", "no_truncation", "no_fp16")}

# winner, its weight, weight minus the runner-up's (inf without one), the sum of all addends and their number
Vote = namedtuple("Vote", "id weight margin total n")


def gamma(n, u):
    """Higham's gamma_n: the relative error bound of a chain of n roundings."""
    return n * u / (1.0 - n * u)


def f16(x):
    """Round to fp16 (to nearest even, one rounding), as float64."""
    return np.asarray(x).astype(np.float16).astype(np.float64)


def window(cs, S, T, rules=RULES):
    """x[cs : cs + S] of a length-T sequence -> (start, length)."""
    if rules.wrap_negative:
        a, b, _ = slice(cs, cs + S).indices(T)
    else:
        a, b = min(max(cs, 0), T), min(max(cs + S, 0), T)
    return a, max(b - a, 0)


def _pairs(S, cs, T, rules):
    """(frame index, attention index) pairs of one token, in the reference's loop order."""
    a, n = window(int(cs), S, T, rules)
    fr = list(range(a, a + n))
    if not rules.truncate and n > 0:
        fr += [a + n - 1] * (S - n)
    return fr, list(range(len(fr)))


def _decide(items, tie, literal, n, empty_weight):
    """items: (id, weight) in insertion order.  `literal` is the reference's own expression, used under the right rule."""
    if not items:
        return Vote(-1, empty_weight, INF, 0.0, 0)
    top = max(w for _, w in items)
    tied = [i for i, w in items if w == top]
    win = ({"first": tied[0], "last": tied[-1], "lowest": min(tied)}[tie], top)
    if literal is not None:       # the rule's name means what the reference's expression does
        assert tuple(literal(items)) == win, (literal(items), win)
        win = literal(items)
    ws = sorted(w for _, w in items)
    return Vote(win[0], win[1], ws[-1] - ws[-2] if len(ws) > 1 else INF, float(sum(ws)), n)


def vote(attn, cs, ids, rules=RULES):
    """Per token: the speaker id with the largest summed attention inside the window; max() over the dict's insertion order."""
    T, S = len(ids), attn.shape[1]
    out = []
    for n in range(attn.shape[0]):
        w = {}
        fr, ai = _pairs(S, cs[n], T, rules)
        for p, s in zip(fr, ai):
            sid = int(ids[p])
            w[sid] = w.get(sid, 0.0) + float(attn[n, s])
        literal = (lambda it: max(it, key=lambda kv: kv[1])) if rules.tie_vote == "first" else None
        out.append(_decide(list(w.items()), rules.tie_vote, literal, len(fr), -INF))
    return out


def vote_groups(attn, cs, ids, offsets, num_ids, half, rules=RULES):
    """Per group of tokens: speaker_weights[sid] += w.item() over tokens, then frames (:158-169); the winner is
    sorted(speaker_weights.items(), key=weight)[-1] (:195-196)."""
    T, S = len(ids), attn.shape[1]
    a = np.asarray(attn, dtype=np.float32)
    a = f16(a) if half and rules.round_fp16 else a.astype(np.float64)
    out = []
    for g in range(len(offsets) - 1):
        w, n = {}, 0
        for t in range(int(offsets[g]), int(offsets[g + 1])):
            fr, ai = _pairs(S, cs[t], T, rules)
            for p, s in zip(fr, ai):
                sid = int(ids[p])
                if rules.ignore_out_of_range and not 0 <= sid < num_ids:
                    continue
                w[sid] = w.get(sid, 0.0) + float(a[t, s])
                n += 1
        literal = (lambda it: sorted(it, key=lambda kv: kv[1])[-1]) if rules.tie_groups == "last" else None
        out.append(_decide(list(w.items()), rules.tie_groups, literal, n, 0.0))
    return out


def majority(ids, ranges, num_ids, rules=RULES):
    """Counter(ids[a:b]).most_common(1) per range (:330-333); weight = the count."""
    lst = [int(i) for i in ids]
    out = []
    for a, b in ranges:
        a, b = int(a), int(b)
        seg = lst[a:b] if rules.wrap_negative else lst[max(a, 0):max(b, 0)]
        if rules.ignore_out_of_range:
            seg = [i for i in seg if 0 <= i < num_ids]
        c = Counter(seg)
        literal = (lambda it: c.most_common(1)[0]) if rules.tie_major == "first" else None
        v = _decide(list(c.items()), rules.tie_major, literal, len(seg), 0.0)
        out.append(v._replace(weight=float(v.weight), margin=float(v.margin)))
    return out


def pool(attn, cs, feat, half, rules=RULES):
    """emb[n] = attention[n, :len] @ features[window(n)] as the float64 dot product of the operands (the fp16-rounded ones in
    half mode) -> (exact [N, E], sum |a * f| [N, E], window lengths [N])."""
    a = np.asarray(attn, dtype=np.float32)
    f = np.asarray(feat, dtype=np.float32)
    if half and rules.round_fp16:
        a, f = f16(a), f16(f)
    else:
        a, f = a.astype(np.float64), f.astype(np.float64)
    N, S = a.shape
    T, E = f.shape
    exact, mag, lens = np.zeros((N, E)), np.zeros((N, E)), np.zeros(N, dtype=np.int64)
    for n in range(N):
        fr, ai = _pairs(S, cs[n], T, rules)
        lens[n] = len(fr)
        if fr:
            exact[n] = a[n, ai] @ f[fr]
            mag[n] = np.abs(a[n, ai]) @ np.abs(f[fr])
    return exact, mag, lens


# ------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------
def window_starts(T, S):
    """Chunk starts that reach every form of the python slice x[cs : cs + S] for a length-T sequence, forwards and backwards."""
    w = [0, T - S, T - S + 1, T - 1, T, T + 5, -1, -57, -S, -S - 1, -T - S - 3]
    return np.asarray(w + w[::-1], dtype=np.int64)


GROUP_OFFSETS = np.asarray([0, 1, 4, 4, 9, 11, 22], dtype=np.int64)      # one token, several, none, the rest


def major_ranges(T):
    return np.asarray([[0, 10], [7, 7], [10, 5], [-20, 400], [-5, -1], [T - 1, T + 100], [-T - 10, 3], [0, T], [100, 700]],
                      dtype=np.int64)


def exact_attn(rng, N, S, hi=2048):
    """Multiples of 2^-12 below 0.5 (11 significant bits: fp16 values too): every fp32 / float64 sum of them is exact in any order."""
    return (rng.randint(0, hi, size=(N, S)) / 4096.0).astype(np.float32)


def random_attn(rng, N, S):
    a = rng.rand(N, S).astype(np.float32) ** 6
    return (a / a.sum(-1, keepdims=True)).astype(np.float32)


def id_pool(rng, num_ids, k=12):
    """A dozen ids spread over [0, num_ids), with both ends of the table."""
    return np.unique(np.concatenate([rng.randint(0, num_ids, size=k), [0, num_ids - 1]])).astype(np.int32)


def _windows_case(kind, T, S, seed, exact=True, num_ids=9, E=None, n_values=9):
    def make():
        rng = np.random.RandomState(seed)
        cs = window_starts(T, S)
        N = len(cs)
        c = dict(T=T, S=S, N=N, cs=cs, attn=exact_attn(rng, N, S) if exact else random_attn(rng, N, S))
        if kind == "pool":
            c.update(E=E, feat=rng.randn(T, E).astype(np.float32))
        else:
            c["ids"] = rng.randint(0, n_values, size=T).astype(np.int32)
        if kind == "groups":
            c.update(num_ids=num_ids, offsets=GROUP_OFFSETS)
        return c
    name = "%s_windows_T%d_S%d" % (kind, T, S) + ("_E%d" % E if E else "") + ("" if exact or kind == "pool" else "_random")
    return dict(name=name, kind=kind, exact=exact and kind != "pool", make=make, must=())


def _vote_ties():
    S = 600
    rows = []            # (first position of A, of B, id A, id B): A and B tie, A appears first
    for pa, pb in ((3, 259), (3, 515), (3, 40), (3, 130), (300, 556), (300, 580)):   # same thread (one, two wraps), lanes, waves
        rows += [(pa, pb, 2, 5), (pa, pb, 5, 2)]

    def make():
        n_rows = len(rows) + 3
        ids = np.tile(100 + np.arange(S) % 50, n_rows).astype(np.int32)
        attn = np.tile(((1 + np.arange(S) % 3) / 4096.0).astype(np.float32), (n_rows + 1, 1))
        for r, (pa, pb, ia, ib) in enumerate(rows):
            ids[r * S + pa], ids[r * S + pa + 7], ids[r * S + pb], ids[r * S + pb + 9] = ia, ia, ib, ib
            attn[r, [pa, pa + 7, pb, pb + 9]] = (0.25, 0.125, 0.125, 0.25)
        r = len(rows)                                    # three ids tie: lanes, waves and the strided loop in one row
        for p, i in ((3, 5), (70, 2), (259, 7)):
            ids[r * S + p], ids[r * S + p + 1] = i, i
            attn[r, [p, p + 1]] = 0.125
        attn[r + 1] = 0.0                                # all-zero row: every id ties at 0
        attn[r + 2, :] = 0.0                             # fifty ids tie above zero, one per position class
        attn[r + 2, :50] = 0.25
        cs = np.arange(n_rows + 1, dtype=np.int64) * S   # the last row's window is empty (start = T)
        return dict(T=n_rows * S, S=S, N=n_rows + 1, cs=cs, attn=attn, ids=ids)
    return dict(name="vote_ties", kind="vote", exact=True, make=make, must=("vote_tie_last", "vote_tie_lowest"))


TIE_IDS = ((7, 263), (263, 7), (7, 40), (40, 7), (7, 130), (130, 7))   # same thread of the table scan, lanes of a wave, waves


def _groups_ties():
    S, num_ids = 64, 300

    def make():
        G = len(TIE_IDS) + 6
        n_tok = 2 * G
        ids = np.tile(200 + np.arange(S) % 20, n_tok).astype(np.int32)
        attn = np.tile(((1 + np.arange(S) % 3) / 4096.0).astype(np.float32), (n_tok, 1))
        cs = np.arange(n_tok, dtype=np.int64) * S
        offsets = 2 * np.arange(G + 1, dtype=np.int64)
        for g, (x, y) in enumerate(TIE_IDS):             # x appears first, y second; both sum to 0.375 over the two tokens
            t0, t1 = 2 * g, 2 * g + 1
            ids[t0 * S + 5], ids[t0 * S + 20], ids[t1 * S + 9], ids[t1 * S + 3] = x, y, x, y
            attn[t0, 5], attn[t0, 20], attn[t1, 9], attn[t1, 3] = 0.25, 0.125, 0.125, 0.25
        g = len(TIE_IDS)                                 # four ids tie across thread, lane and wave
        for k, i in enumerate((7, 130, 263, 40)):
            ids[2 * g * S + 4 * k] = i
            attn[2 * g, 4 * k] = 0.375
        attn[2 * (g + 1):2 * (g + 2)] = 0.0              # all-zero group: every id ties at 0
        offsets[g + 3:] -= 2                             # group g + 2 is empty (no tokens) ...
        cs[offsets[g + 3]:offsets[g + 4]] = n_tok * S    # ... the next has tokens with empty windows only (start = T) ...
        t = int(offsets[g + 4])                          # ... the next only ids outside [0, num_ids) ...
        ids[t * S:(t + 2) * S] = np.where(np.arange(2 * S) % 2, -1, num_ids)
        t = int(offsets[g + 5])                          # ... and the last has them with the largest weights beside real ids
        ids[t * S + 1], ids[t * S + 2], ids[t * S + 40] = -1, num_ids, 299
        attn[t, 1], attn[t, 2], attn[t, 40] = 0.45, 0.45, 0.125
        n_used = int(offsets[-1])
        return dict(T=n_tok * S, S=S, N=n_used, cs=cs[:n_used], attn=attn[:n_used], ids=ids, offsets=offsets, num_ids=num_ids)
    return dict(name="groups_ties", kind="groups", exact=True, make=make,
                must=("groups_tie_first", "groups_tie_lowest", "count_out_of_range"))


def _groups_half():
    """fp32 attention makes one id win, its fp16 rounding another (group 0) or a tie (group 1)."""
    def make():
        S, u = 16, 2.0 ** -14                            # fp16 spacing in [1/16, 1/8)
        x0 = 1638 * u
        ids = np.tile(np.arange(S) % 4 + 10, 2).astype(np.int32)
        attn = np.zeros((2, S), dtype=np.float32)
        ids[[0, 1, 2]] = 3                               # id 3: three values that round up -> 3 x0 + 3 u (fp32: 3 x0 + 1.8 u)
        attn[0, [0, 1, 2]] = x0 + 0.6 * u
        ids[[5, 6, 7]] = 8                               # id 8: 3 x0 + 2.45 u in fp32 (wins), 3 x0 + 2 u once rounded (loses)
        attn[0, [5, 6, 7]] = (x0 + 1.45 * u, x0 + 1.45 * u, x0 - 0.45 * u)
        ids[S + 2], ids[S + 9] = 4, 6                    # id 4 appears first and is larger in fp32; rounded, both are 0.5: 6 wins
        attn[1, 2], attn[1, 9] = 0.5 + 2.0 ** -12, 0.5 + 2.0 ** -13
        return dict(T=2 * S, S=S, N=2, cs=np.asarray([0, S], dtype=np.int64), attn=attn, ids=ids,
                    offsets=np.asarray([0, 1, 2], dtype=np.int64), num_ids=20)
    return dict(name="groups_half_rounding", kind="groups", exact=True, make=make, must=("no_fp16",))


def _groups_num_ids(num_ids, seed):
    T, S = 1000, 357

    def make():
        rng = np.random.RandomState(seed)
        cs = window_starts(T, S)
        N = len(cs)
        pool_ids = id_pool(rng, num_ids)
        ids = pool_ids[rng.randint(0, len(pool_ids), size=T)]
        ids[rng.rand(T) < 0.1] = -1
        ids[rng.rand(T) < 0.1] = num_ids
        ids[T - S:T - S + 40] = num_ids - 1              # the last entry of the table wins the second group
        return dict(T=T, S=S, N=N, cs=cs, attn=exact_attn(rng, N, S), ids=ids.astype(np.int32), num_ids=num_ids,
                    offsets=GROUP_OFFSETS)
    return dict(name="groups_num_ids_%d" % num_ids, kind="groups", exact=True, make=make, must=())


def _major_windows(T, seed, num_ids=5):
    def make():
        rng = np.random.RandomState(seed)
        pool_ids = id_pool(rng, num_ids, 4) if num_ids > 5 else np.arange(num_ids, dtype=np.int32)
        ids = pool_ids[rng.randint(0, len(pool_ids), size=T)]
        if num_ids != 5:
            ids[rng.rand(T) < 0.1] = -1
            ids[rng.rand(T) < 0.1] = num_ids
            ids[max(T - 5, 0):T] = num_ids - 1           # the table's last entry wins [-5, -1] and [T - 1, T + 100]
        return dict(T=T, ids=ids.astype(np.int32), ranges=major_ranges(T), num_ids=num_ids)
    name = "major_windows_T%d" % T if num_ids == 5 else "major_num_ids_%d" % num_ids
    return dict(name=name, kind="major", exact=True, make=make, must=())


def _major_ties():
    num_ids, L = 300, 40

    def make():
        segs, ranges = [], []

        def add(seg):
            a = sum(len(s) for s in segs)
            segs.append(np.asarray(seg, dtype=np.int32))
            ranges.append([a, a + len(seg)])
        for x, y in TIE_IDS:                             # x appears first; two each, every other id once
            add([x, y, y, x] + list(range(200, 200 + L - 4)))
        for x, y in ((7, 263), (263, 7)):                # first appearances 295 apart: another pass of the strided loop
            seg = 8 + np.arange(600) % 250               # (every filler at most three times, x and y four times each)
            seg[[5, 400, 401, 402]] = x
            seg[[300, 301, 302, 599]] = y
            add(seg)
        add(list(range(299, 299 - L, -1)))               # all ids once: every id ties
        add([-1, num_ids] * 5)                           # only ids outside [0, num_ids)
        add([-1, -1, -1, num_ids, num_ids, num_ids, 17, 17, 4])   # ... outnumbering the real ones
        ids = np.concatenate(segs)
        ranges.append([len(ids), len(ids) + 5])          # empty range
        return dict(T=len(ids), ids=ids, ranges=np.asarray(ranges, dtype=np.int64), num_ids=num_ids)
    return dict(name="major_ties", kind="major", exact=True, make=make,
                must=("major_tie_last", "major_tie_lowest", "count_out_of_range"))


def _vote_largest_s():
    """S = 8192, the most tal_attn_vote_fwd accepts: 64 KB of dynamic LDS beside the kernel's static 48 bytes."""
    def make():
        rng = np.random.RandomState(81)
        T, S = 9000, 8192
        ids = rng.randint(0, 40, size=T).astype(np.int32)
        attn = exact_attn(rng, 3, S, hi=4)
        ids[S - 1] = 77                                  # the first row's winner sits in the last LDS slot
        attn[0, S - 1] = 2007 / 4096.0
        return dict(T=T, S=S, N=3, cs=np.asarray([0, T - S, 5000], dtype=np.int64), attn=attn, ids=ids)
    return dict(name="vote_largest_S_8192", kind="vote", exact=True, make=make, must=())


def _pool_single():
    def make():
        rng = np.random.RandomState(5)
        return dict(T=1000, S=357, N=1, E=128, cs=np.asarray([321], dtype=np.int64), attn=random_attn(rng, 1, 357),
                    feat=rng.randn(1000, 128).astype(np.float32))
    return dict(name="pool_single_token", kind="pool", exact=False, make=make, must=())


CASES = [
    # per-token vote: every window form at every S (one pass, a partial pass, two and three passes of the 256-thread loops)
    _windows_case("vote", 1000, 357, 1), _windows_case("vote", 300, 357, 2), _windows_case("vote", 1, 1, 3),
    _windows_case("vote", 1, 64, 4), _windows_case("vote", 1000, 1, 5), _windows_case("vote", 1000, 64, 6),
    _windows_case("vote", 1000, 257, 7), _windows_case("vote", 1000, 600, 8), _windows_case("vote", 300, 600, 9),
    _windows_case("vote", 1000, 357, 10, exact=False, n_values=7), _windows_case("vote", 1000, 600, 11, exact=False, n_values=7),
    _vote_ties(), _vote_largest_s(),
    # grouped vote
    _windows_case("groups", 1000, 357, 21), _windows_case("groups", 300, 357, 22), _windows_case("groups", 1, 1, 23),
    _windows_case("groups", 1000, 64, 24), _windows_case("groups", 1000, 257, 25), _windows_case("groups", 1000, 600, 26),
    _windows_case("groups", 300, 600, 27), _windows_case("groups", 1000, 357, 28, exact=False),
    _windows_case("groups", 300, 600, 29, exact=False),
    _groups_ties(), _groups_half(),
    # (5455 .. 5461: 12 * num_ids + 8 bytes of dynamic LDS and the 64 static ones cross 64 KB between 5455 and 5456,
    # the dynamic part alone between 5460 and 5461)
    _groups_num_ids(1, 31), _groups_num_ids(9, 32), _groups_num_ids(300, 33), _groups_num_ids(6008, 34),
    _groups_num_ids(13631, 35), _groups_num_ids(5455, 36), _groups_num_ids(5456, 37), _groups_num_ids(5460, 38),
    _groups_num_ids(5461, 39),
    # majority vote
    _major_windows(1000, 41), _major_windows(300, 42), _major_windows(1, 43), _major_ties(),
    _major_windows(1000, 44, num_ids=1), _major_windows(1000, 45, num_ids=9), _major_windows(1000, 46, num_ids=300),
    _major_windows(1000, 47, num_ids=6008), _major_windows(1000, 48, num_ids=13631), _major_windows(1000, 49, num_ids=5455),
    _major_windows(1000, 50, num_ids=5456), _major_windows(1000, 51, num_ids=5460), _major_windows(1000, 52, num_ids=5461),
    # pooling
    _windows_case("pool", 1000, 357, 61, E=1), _windows_case("pool", 1000, 357, 62, E=127), _windows_case("pool", 1000, 357, 63, E=128),
    _windows_case("pool", 1000, 357, 64, E=129), _windows_case("pool", 1000, 357, 65, E=300), _windows_case("pool", 300, 357, 66, E=128),
    _windows_case("pool", 1, 1, 67, E=1), _windows_case("pool", 1000, 1, 68, E=128), _windows_case("pool", 1000, 64, 69, E=127),
    _windows_case("pool", 1000, 257, 70, E=300), _windows_case("pool", 1000, 600, 71, E=129), _windows_case("pool", 300, 600, 72, E=128),
    _pool_single(),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


@lru_cache(maxsize=None)
def inputs(name):
    """The case's arrays; generated once and shared (callers must not write to them)."""
    c = CASE_BY_NAME[name]["make"]()
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def modes(case):
    """half_mode values the case runs with."""
    return (0, 1) if case["kind"] in ("groups", "pool") else (0,)


@lru_cache(maxsize=None)
def _model(name, mode, rules):
    case, c = CASE_BY_NAME[name], inputs(name)
    kind = case["kind"]
    if kind == "vote":
        return vote(c["attn"], c["cs"], c["ids"], rules)
    if kind == "groups":
        return vote_groups(c["attn"], c["cs"], c["ids"], c["offsets"], c["num_ids"], mode, rules)
    if kind == "major":
        return majority(c["ids"], c["ranges"], c["num_ids"], rules)
    return pool(c["attn"], c["cs"], c["feat"], mode, rules)


def model(case, mode, rules=RULES):
    return _model(case["name"], mode, rules)


def outputs(case, mode, rules=RULES):
    """What a kernel that follows `rules` without rounding error returns: {"id", "weight"} or {"out"}."""
    m = model(case, mode, rules)
    if case["kind"] == "pool":
        return {"out": f16(m[0]) if mode else m[0].copy()}
    return {"id": np.asarray([v.id for v in m], dtype=np.int64), "weight": np.asarray([v.weight for v in m], dtype=np.float64)}


def vote_unit(case):
    """Unit roundoff of the kernel's sums: the per-token vote adds in fp32, the group kernels in float64."""
    return U32 if case["kind"] == "vote" else U64


def weights_exact(case, mode):
    """The kernel's weights must equal the model's bit for bit: exact-valued cases, counts, and the grouped vote in half mode
    (fp16 addends: float64 sums of them are exact in any order)."""
    return case["exact"] or case["kind"] == "major" or (case["kind"] == "groups" and mode == 1)


def compare(case, mode, got):
    """Assert that `got` (as outputs()) is what the right rules give, to the derived bounds."""
    m = model(case, mode)
    if case["kind"] == "pool":
        exact, mag, lens = m
        out = np.asarray(got["out"], dtype=np.float64)
        assert out.shape == exact.shape and np.all(np.isfinite(out)), case["name"]
        b = np.asarray([gamma(max(int(n), 1), U32) for n in lens])[:, None] * mag     # one fmaf chain of len terms
        if mode:
            lo, hi = f16(exact - b), f16(exact + b)
            assert np.array_equal(out, f16(out)), "%s: half mode returned values that are not fp16 numbers" % case["name"]
        else:
            lo, hi = exact - b, exact + b
        bad = (out < lo) | (out > hi)
        i = int(np.argmax(np.abs(out - exact) - b))
        assert not bad.any(), "%s mode %d: %d outputs outside the bound; worst at flat index %d: got %r, exact %r, bound %.3g" % (
            case["name"], mode, int(bad.sum()), i, out.flat[i], exact.flat[i], b.flat[i])
        return
    ids, wts = np.asarray(got["id"]), np.asarray(got["weight"], dtype=np.float64)
    assert len(ids) == len(m) and len(wts) == len(m), case["name"]
    u = vote_unit(case)
    for k, v in enumerate(m):
        assert int(ids[k]) == v.id, "%s mode %d row %d: id %d, the model has %d (weight %r, margin %r)" % (
            case["name"], mode, k, int(ids[k]), v.id, v.weight, v.margin)
        if weights_exact(case, mode) or v.id < 0:
            assert wts[k] == v.weight, "%s mode %d row %d: weight %r, the model has %r" % (case["name"], mode, k, wts[k], v.weight)
        else:
            tol = 2 * gamma(v.n, u) * v.total
            assert abs(wts[k] - v.weight) <= tol, "%s mode %d row %d: weight %r, the model has %r, bound %.3g" % (
                case["name"], mode, k, wts[k], v.weight, tol)
