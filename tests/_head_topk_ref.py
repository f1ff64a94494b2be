"""Float64 model of the per-row top-k / log-sum-exp of the speaker head (tal_spk_topk_fwd, tal_topk_lse_rows), the case table the
CPU and GPU tests share, and the comparison with its error bound.

Semantics (include/tal_asrd.h): z[r, s] = feat[r, :] . W[s, :] + b[s], lse[r] = log sum_s exp(z[r, s]); ids = the k largest z per row,
value descending and index ascending among equal values; logp = z[ids] - lse.  A -inf bias masks a column: nothing in lse, ranked
below every finite column (by index among its kind), logp = -inf.

Error bound, u = 2^-24, gamma_n = n u / (1 - n u):
  B[r, s] = gamma_{E+2} (sum_k |feat[r, k]| |W[s, k]| + |b[s]|) bounds an fp32 logit (E products, E - 1 additions, the bias) in any
  order of summation.  lse is 1-Lipschitz in the sup norm of the logits and an fp32 sum of S positive terms has at most gamma_S
  relative error, so |lse - exact| <= max_s B[r, s] + (S + 64) u (the 64 u cover the exp / log evaluations) and
  |logp - exact| <= B[r, s] + max_s B[r, s] + (S + 64) u.
Ids: a row is CLEAR when every adjacent gap among its exact top-(k+1) logits exceeds 2 max_s B[r, s]: fp32 rounding cannot change the
order there and the ids must be the model's.  On any other row every returned id's exact logit must reach the exact k-th minus
2 max_s B.  Exact-valued cases (small-integer features, weights and biases multiples of 2^-4: every partial sum is exact in fp32 in any
order) must match the model's ids on EVERY row, ties included.
"""
import functools

import numpy as np
import torch

U = 2.0 ** -24
E = 128
UNCLEAR_CAP = 0.05          # a random case may have at most this share of unclear rows

VARIANTS = ("tie_reversed", "last_tile_dropped", "sum_not_rescaled", "bias_not_ranked", "inf_poisons_sum", "kth_off_by_one")


def gamma(n):
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------ the model
def _order(z, reverse_ties=False):
    """Per row: column indices by value descending, index ascending among equal values (descending with reverse_ties)."""
    if reverse_ties:
        n = z.shape[1]
        return n - 1 - np.argsort(-z[:, ::-1], axis=1, kind="stable")
    return np.argsort(-z, axis=1, kind="stable")


def _lse(z):
    m = z.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        return (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))[:, 0]


def topk_lse(z, k, variant=None, zrank=None):
    """z [M, S] float64 (may hold -inf) -> ids [M, k], logp [M, k], lse [M].  variant: one of VARIANTS, a plausible wrong kernel."""
    z = np.asarray(z, dtype=np.float64)
    S = z.shape[1]
    rank = z if zrank is None or variant != "bias_not_ranked" else zrank
    lse_src = z
    if variant == "last_tile_dropped" and S % 128 and S > 128:
        keep = S - S % 128
        rank, lse_src = rank[:, :keep], z[:, :keep]
    order = _order(rank, reverse_ties=variant == "tie_reversed")
    if variant == "kth_off_by_one" and order.shape[1] > k:
        ids = np.concatenate([order[:, :k - 1], order[:, k:k + 1]], axis=1)
    else:
        ids = order[:, :k]
    if variant == "sum_not_rescaled":
        # per 128-column slot (max, sum of exp(z - max)); the sums added as they are under the largest max
        nt = -(-S // 128)
        ms = [z[:, t * 128:(t + 1) * 128].max(axis=1) for t in range(nt)]
        with np.errstate(invalid="ignore"):
            ss = [np.where(np.isfinite(ms[t]), np.exp(z[:, t * 128:(t + 1) * 128] - ms[t][:, None]).sum(axis=1), 0.0) for t in range(nt)]
        lse = np.max(ms, axis=0) + np.log(np.sum(ss, axis=0))
    elif variant == "inf_poisons_sum":
        with np.errstate(invalid="ignore"):
            lse = _lse(lse_src) + np.where(np.isinf(z).any(axis=1), np.nan, 0.0)     # exp(-inf - -inf) somewhere in the sum
    else:
        lse = _lse(lse_src)
    with np.errstate(invalid="ignore"):
        logp = np.take_along_axis(z, ids, axis=1) - lse[:, None]
    return ids.astype(np.int64), logp, lse


class Ref:
    """The exact results of a case and what `compare` needs: z, B, ids, logp, lse, clear rows."""

    def __init__(self, z, B, k, exact_valued, zrank=None):
        self.z, self.B, self.k, self.exact_valued, self.zrank = z, B, k, exact_valued, zrank
        self.M, self.S = z.shape
        self.ids, self.logp, self.lse = topk_lse(z, k)
        self.Bmax = np.where(np.isfinite(z), B, 0.0).max(axis=1)
        top = -np.sort(-z, axis=1)[:, :min(k + 1, self.S)]
        with np.errstate(invalid="ignore"):
            gaps = top[:, :-1] - top[:, 1:]          # -inf next to -inf: NaN -- both are exact in fp32, their order is by index
        self.clear = np.all(np.isnan(gaps) | (gaps > 2 * self.Bmax[:, None]), axis=1) if gaps.shape[1] else np.ones(self.M, bool)
        self.kth = np.take_along_axis(z, self.ids[:, -1:], axis=1)[:, 0]

    @property
    def unclear_share(self):
        return 1.0 - self.clear.mean()

    def wrong(self, variant):
        return topk_lse(self.z, self.k, variant=variant, zrank=self.zrank)


def linear_ref(feat, W, b, k, exact_valued=False):
    f, w = feat.astype(np.float64), W.astype(np.float64)
    bb = np.zeros(W.shape[0]) if b is None else b.astype(np.float64)
    zr = f @ w.T
    z = zr + bb
    B = gamma(feat.shape[1] + 2) * (np.abs(f) @ np.abs(w).T + np.where(np.isfinite(bb), np.abs(bb), 0.0))
    return Ref(z, B, k, exact_valued, zrank=zr)


def rows_ref(x, k, exact_valued=False):
    """tal_topk_lse_rows: the matrix is given, only the sum and the subtraction round."""
    return Ref(x.astype(np.float64), np.zeros(x.shape), k, exact_valued)


def compare(ref, ids, logp, lse):
    """-> list of messages, empty when (ids [M, k], logp [M, k], lse [M]) is within the bound of the model."""
    ids, logp, lse = np.asarray(ids).astype(np.int64), np.asarray(logp, dtype=np.float64), np.asarray(lse, dtype=np.float64)
    bad = []
    if ids.shape != ref.ids.shape or logp.shape != ref.ids.shape or lse.shape != (ref.M,):
        return ["shapes %s %s %s" % (ids.shape, logp.shape, lse.shape)]
    if ids.min() < 0 or ids.max() >= ref.S:
        return ["id out of range [%d, %d]" % (ids.min(), ids.max())]
    if any(len(set(r)) != ref.k for r in ids.tolist()):
        bad.append("repeated id in a row")
    slack = (ref.S + 64) * U
    lse_err = np.abs(lse - ref.lse)
    if not np.all(lse_err <= ref.Bmax + slack):
        r = int(np.argmax(np.where(np.isnan(lse_err), np.inf, lse_err - ref.Bmax)))
        bad.append("lse row %d: %r vs %r (bound %.3e)" % (r, lse[r], ref.lse[r], ref.Bmax[r] + slack))
    must = np.ones(ref.M, bool) if ref.exact_valued else ref.clear
    wrong = must & np.any(ids != ref.ids, axis=1)
    if wrong.any():
        r = int(np.argmax(wrong))
        bad.append("ids row %d (%d rows): %s vs %s" % (r, wrong.sum(), ids[r].tolist(), ref.ids[r].tolist()))
    zg = np.take_along_axis(ref.z, ids, axis=1)
    if not np.all(zg >= (ref.kth - 2 * ref.Bmax)[:, None]):
        r = int(np.argmax(np.any(~(zg >= (ref.kth - 2 * ref.Bmax)[:, None]), axis=1)))
        bad.append("row %d returns an id below the k-th logit: %s" % (r, ids[r].tolist()))
    with np.errstate(invalid="ignore"):
        want = zg - ref.lse[:, None]
        err = np.abs(logp - want)
    fin = np.isfinite(want)
    bound = np.take_along_axis(ref.B, ids, axis=1) + ref.Bmax[:, None] + slack
    if not np.all(np.where(fin, err <= bound, logp == want)):
        r = int(np.argmax(np.any(~np.where(fin, err <= bound, logp == want), axis=1)))
        bad.append("logp row %d: %s vs %s" % (r, logp[r].tolist(), want[r].tolist()))
    return bad


# ------------------------------------------------------------------ the cases
def _random_inputs(M, S, seed=None):
    """The recipe of test_long_input_argmax_head_matches_logits_argmax's head: O(1) features, logits of a few units."""
    g = torch.Generator().manual_seed(M + S if seed is None else seed)
    feat = torch.randn(M, E, generator=g)
    W = torch.randn(S, E, generator=g) / 11
    b = torch.randn(S, generator=g)
    return feat.numpy(), W.numpy(), b.numpy()


def _exact_inputs(M, S, plants, lift):
    """Features in {-2..2}, weights and biases multiples of 2^-4 in [-1/4, 1/4] ([-1, 1]): logits are multiples of 2^-4 of a few
    units, exact in fp32 in any order, with ties at every rank.  The columns of `plants` share one weight row and one bias `lift`
    above it: equal in every row (winners when lift is large)."""
    rng = np.random.RandomState(1000 * M + S)
    feat = rng.randint(-2, 3, size=(M, E)).astype(np.float32)
    W = (rng.randint(-4, 5, size=(S, E)) / 16.0).astype(np.float32)
    b = (rng.randint(-16, 17, size=S) / 16.0).astype(np.float32)
    plants = [c for c in plants if 0 <= c < S]
    for c in plants[1:]:
        W[c] = W[plants[0]]
    for c in plants:
        b[c] = lift
    return feat, W, b


def _plants(S):
    """Equal winners: one lane's column class (3, 7: the lane of columns 0..15 of a 32-column sub-tile; 3, 35 across sub-tiles), the
    two lane halves of a row (3, 19), sub-tiles and N tiles (35, 131), the first / last tile of a 6008-wide head (other workgroup slots
    at a small grid), the edges 0, 31 / 32, 127 / 128, S - 1 and the ragged last tile."""
    last = S - S % 128 if S % 128 else S - 128
    return sorted({0, 3, 7, 19, 31, 32, 35, 127, 128, 131, last + 2, S - 1} & set(range(S)))


MS = (1, 31, 32, 33, 127, 128, 129, 300)
SS = (5, 32, 33, 127, 128, 129, 300, 6008)
KS = (1, 2, 4, 8, 16)


def _case_table():
    cases = {}

    def add(kind, M, S, k, **kw):
        name = "%s-%d-%d-%d%s" % (kind, M, S, k, kw.pop("tag", ""))
        cases[name] = dict(kind=kind, M=M, S=S, k=k, **kw)

    # every (M, S), (M, k) and (S, k) pair once; kinds alternate along both axes
    for i, M in enumerate(MS):
        for j, S in enumerate(SS):
            k = KS[(i + j) % 5]
            while k > S:
                k //= 2
            # (k = 16 leaves 17 gaps to clear 2 max B: the float64 model alone finds 9 % / 8 % unclear rows on random data at
            #  these two shapes, above the cap, so they are exact-valued; the other k = 16 shapes stay random at 0 %)
            crowded = (M, S, k) in ((33, 32, 16), (300, 6008, 16))
            add("exact" if (i + j) % 2 or crowded else "random", M, S, k)
    # the shapes whose unclear share the float64 model gives in the issue; (300, 6008): 141 units, 1 to 4 workgroups on a row block
    for M, S, k in ((300, 6008, 8), (300, 6008, 4), (129, 300, 8), (129, 129, 8), (33, 33, 8)):
        add("random", M, S, k)
    add("exact", 300, 6008, 8)
    add("exact", 300, 6008, 16)
    add("exact", 129, 300, 4)
    # two equal maxima far above the rest (first and last tile): lse = z + ln 2; a dropped column or slot is an error of ln 2
    add("exact", 300, 6008, 2, plants=(37, 6003), lift=64.0, tag="-two")
    add("exact", 33, 300, 1, plants=(37, 295), lift=64.0, tag="-two")
    # masked speakers
    add("masked", 33, 300, 8, finite=(7, 130, 299), tag="-three")
    add("masked", 129, 6008, 4, finite=(5999,), tag="-one")
    add("masked", 129, 6008, 8, masked=tuple(range(5990, 6008)) + (0, 64, 4000), tag="-ragged")
    return cases


CASES = _case_table()
REPEAT_CASE = ("random", 2000, 6008, 8)         # repeatability (and the cap of the issue's table); not in the per-form sweep
ROWS_CASES = {"%s-%d-%d" % (kind, n, k): (kind, 37, n, k)
              for kind in ("random", "exact") for n, k in ((1, 1), (63, 8), (64, 16), (65, 4), (6008, 8))}


@functools.lru_cache(maxsize=None)
def build(name):
    """-> (feat, W, b, Ref) of a head case; computed once per process, treat as read-only."""
    c = CASES[name]
    M, S, k = c["M"], c["S"], c["k"]
    if c["kind"] == "exact":
        lift = c.get("lift", 24.0)
        feat, W, b = _exact_inputs(M, S, c.get("plants", _plants(S)), lift)
    else:
        feat, W, b = _random_inputs(M, S)
        if c["kind"] == "masked":
            b = b.copy()
            if "finite" in c:
                keep = np.zeros(S, bool)
                keep[list(c["finite"])] = True
                b[~keep] = -np.inf
            else:
                b[list(c["masked"])] = -np.inf
    return feat, W, b, linear_ref(feat, W, b, k, exact_valued=c["kind"] == "exact")


@functools.lru_cache(maxsize=None)
def build_repeat():
    kind, M, S, k = REPEAT_CASE
    feat, W, b = _random_inputs(M, S)
    return feat, W, b, linear_ref(feat, W, b, k)


@functools.lru_cache(maxsize=None)
def build_rows(name):
    kind, M, n, k = ROWS_CASES[name]
    if kind == "exact":
        rng = np.random.RandomState(n)
        x = (rng.randint(-64, 65, size=(M, n)) / 16.0).astype(np.float32)
        if n > 2:
            x[:, n - 1] = x[:, 0] = 8.0           # equal winners at both ends
    else:
        x = torch.randn(M, n, generator=torch.Generator().manual_seed(n)).numpy() * 3
    return x, rows_ref(x, k, exact_valued=kind == "exact")
