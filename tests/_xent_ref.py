"""Float64 model of teacher-forced scoring without the logits (tal_xent_rows_fwd, tal_xent_lse_rows, tal_lm_xent_fwd), the case table
the CPU and GPU tests share, and the comparison with its error bound.

Semantics (include/tal_asrd.h): z[r, s] = feat[r, :] . W[s, :] + b[s], lse[r] = log sum_s exp(z[r, s]), nll[r] = lse[r] - z[r, target[r]],
top1[r] = arg-max_s z[r, s] with the FIRST index among equal values.  target < 0 skips the row (nll = 0.0 exactly, lse / top1 still
written); target >= N gives nll = +inf.  A -inf bias masks a column: nothing in lse, a target on it gives nll = +inf.

Error bound, u = 2^-24, gamma_n = n u / (1 - n u):
  B[r, s] = gamma_{E+2} (sum_k |feat[r, k]| |W[s, k]| + |b[s]|) bounds an fp32 logit (E products, E - 1 additions, the bias) in any
  order of summation.  lse is 1-Lipschitz in the sup norm of the logits and an fp32 sum of N positive terms has at most gamma_N
  relative error, so |lse - exact| <= max_s B[r, s] + (N + 64) u (the 64 u cover the exp / log evaluations) and
  |nll - exact| <= B[r, t] + max_s B[r, s] + (N + 64) u.
top1: a row is CLEAR when its exact top-two gap exceeds 2 max_s B[r, s]: fp32 rounding cannot change the winner there and top1 must be
the model's.  On any other row the exact logit of the returned index must reach the exact maximum minus 2 max_s B.  Exact-valued
cases (small-integer features, weights and biases multiples of 2^-4: every partial sum is exact in fp32 in any order) must match
the model's top1 on EVERY row, ties included.
"""
import functools

import numpy as np
import torch

U = 2.0 ** -24
UNCLEAR_CAP = 0.05          # a random case may have at most this share of unclear rows

VARIANTS = ("last_tile_dropped", "sum_not_rescaled", "target_from_other_partial", "skipped_row_not_zeroed", "tie_last_index",
            "inf_poisons_sum")

FUSED_E = (64, 128)         # feature widths of the fused form
GENERIC_E = (32, 256)       # widths only the generic form takes
NS = (1, 127, 128, 129, 300, 1000)
MS = (1, 31, 33, 131, 257)
PAD = 777.0                 # what the columns behind a row's E features hold when ldf > E


def gamma(n):
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------ the model
def _lse(z):
    m = z.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        return (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))[:, 0]


def _gather(z, target):
    """z[r, target[r]] where the target names a column, -inf elsewhere (never an address outside the row)."""
    n = z.shape[1]
    ok = (target >= 0) & (target < n)
    return np.where(ok, np.take_along_axis(z, np.where(ok, target, 0)[:, None], axis=1)[:, 0], -np.inf)


def xent(z, target, variant=None):
    """z [M, N] float64 (may hold -inf), target [M] int64 -> nll [M], lse [M], top1 [M].  variant: one of VARIANTS, a plausible
    wrong kernel."""
    z = np.asarray(z, dtype=np.float64)
    target = np.asarray(target, dtype=np.int64)
    N = z.shape[1]
    zs = z
    if variant == "last_tile_dropped" and N % 128 and N > 128:
        zs = z[:, :N - N % 128]
    if variant == "tie_last_index":
        top1 = zs.shape[1] - 1 - np.argmax(zs[:, ::-1], axis=1)
    else:
        top1 = np.argmax(zs, axis=1)                 # (first maximum)
    if variant == "sum_not_rescaled":
        # per 128-column slot (max, sum of exp(z - max)); the sums added as they are under the largest max
        nt = -(-N // 128)
        ms = [z[:, t * 128:(t + 1) * 128].max(axis=1) for t in range(nt)]
        with np.errstate(invalid="ignore", over="ignore"):
            ss = [np.where(np.isfinite(ms[t]), np.exp(z[:, t * 128:(t + 1) * 128] - ms[t][:, None]).sum(axis=1), 0.0) for t in range(nt)]
        lse = np.max(ms, axis=0) + np.log(np.sum(ss, axis=0))
    elif variant == "inf_poisons_sum":
        with np.errstate(invalid="ignore"):
            lse = _lse(zs) + np.where(np.isinf(z).any(axis=1), np.nan, 0.0)     # exp(-inf - -inf) somewhere in the sum
    else:
        lse = _lse(zs)
    if variant == "target_from_other_partial":
        zt = _gather(z, np.where((target >= 0) & (target < N), target % 128, target))
    else:
        zt = _gather(zs, target)
    with np.errstate(invalid="ignore"):
        nll = np.where(np.isfinite(zt), lse - zt, np.inf)
    if variant == "skipped_row_not_zeroed":
        nll = np.where(target < 0, lse, nll)
    else:
        nll = np.where(target < 0, 0.0, nll)
    return nll, lse, top1.astype(np.int64)


class Ref:
    """The exact results of a case and what `compare` needs: z, B, target, nll, lse, top1, clear rows."""

    def __init__(self, z, B, target, exact_valued):
        self.z, self.B, self.target, self.exact_valued = z, B, np.asarray(target, dtype=np.int64), exact_valued
        self.M, self.N = z.shape
        self.nll, self.lse, self.top1 = xent(z, self.target)
        self.Bmax = np.where(np.isfinite(z), B, 0.0).max(axis=1)
        if self.N > 1:
            top = -np.sort(-z, axis=1)[:, :2]
            with np.errstate(invalid="ignore"):
                gap = top[:, 0] - top[:, 1]
            self.clear = np.isnan(gap) | (gap > 2 * self.Bmax)       # (-inf next to -inf: both exact, the order is by index)
        else:
            self.clear = np.ones(self.M, bool)
        self.zmax = z.max(axis=1)
        ok = (self.target >= 0) & (self.target < self.N)
        self.Bt = np.where(ok, np.take_along_axis(B, np.where(ok, self.target, 0)[:, None], axis=1)[:, 0], 0.0)

    @property
    def unclear_share(self):
        return 1.0 - self.clear.mean()

    def wrong(self, variant):
        return xent(self.z, self.target, variant=variant)


def linear_ref(feat, W, b, target, exact_valued=False):
    """feat [M, E] (the features alone, without the padding of a pitched row)."""
    f, w = feat.astype(np.float64), W.astype(np.float64)
    bb = np.zeros(W.shape[0]) if b is None else b.astype(np.float64)
    z = f @ w.T + bb
    B = gamma(feat.shape[1] + 2) * (np.abs(f) @ np.abs(w).T + np.where(np.isfinite(bb), np.abs(bb), 0.0))
    return Ref(z, B, target, exact_valued)


def rows_ref(x, target, exact_valued=False):
    """tal_xent_lse_rows: the matrix is given.  What rounds is the sum (the (N + 64) u of `compare`), lse = max + log(sum) and
    nll = lse - x[t]: one rounding each of values no larger than max |x| + log N, which B = 2 u (|x| + log N) per entry covers."""
    x64 = x.astype(np.float64)
    return Ref(x64, 2 * U * (np.where(np.isfinite(x64), np.abs(x64), 0.0) + np.log(x.shape[1]) + 1.0), target, exact_valued)


def compare(ref, nll, lse, top1):
    """-> list of messages, empty when (nll [M], lse [M], top1 [M]) is within the bound of the model."""
    nll, lse, top1 = np.asarray(nll, dtype=np.float64), np.asarray(lse, dtype=np.float64), np.asarray(top1).astype(np.int64)
    bad = []
    if nll.shape != (ref.M,) or lse.shape != (ref.M,) or top1.shape != (ref.M,):
        return ["shapes %s %s %s" % (nll.shape, lse.shape, top1.shape)]
    if top1.min() < 0 or top1.max() >= ref.N:
        return ["top1 out of range [%d, %d]" % (top1.min(), top1.max())]
    slack = (ref.N + 64) * U
    lse_err = np.abs(lse - ref.lse)
    if not np.all(lse_err <= ref.Bmax + slack):
        r = int(np.argmax(np.where(np.isnan(lse_err), np.inf, lse_err - ref.Bmax)))
        bad.append("lse row %d: %r vs %r (bound %.3e)" % (r, lse[r], ref.lse[r], ref.Bmax[r] + slack))
    skipped = ref.target < 0
    if not np.all((nll[skipped] == 0.0)):
        bad.append("a skipped row's nll is not 0.0: %r" % nll[skipped][nll[skipped] != 0.0][:4].tolist())
    fin = np.isfinite(ref.nll) & ~skipped
    with np.errstate(invalid="ignore"):
        ok = np.where(fin, np.abs(nll - ref.nll) <= ref.Bt + ref.Bmax + slack, nll == ref.nll)
    if not np.all(ok):
        r = int(np.argmax(~ok))
        bad.append("nll row %d (target %d, %d rows): %r vs %r (bound %.3e)" % (r, ref.target[r], (~ok).sum(), nll[r], ref.nll[r],
                                                                                ref.Bt[r] + ref.Bmax[r] + slack))
    must = np.ones(ref.M, bool) if ref.exact_valued else ref.clear
    wrong = must & (top1 != ref.top1)
    if wrong.any():
        r = int(np.argmax(wrong))
        bad.append("top1 row %d (%d rows): %d vs %d" % (r, wrong.sum(), top1[r], ref.top1[r]))
    zg = np.take_along_axis(ref.z, top1[:, None], axis=1)[:, 0]
    if not np.all(zg >= ref.zmax - 2 * ref.Bmax):
        r = int(np.argmax(~(zg >= ref.zmax - 2 * ref.Bmax)))
        bad.append("row %d returns a top1 below the maximum: %d" % (r, top1[r]))
    return bad


# ------------------------------------------------------------------ the cases
def _random_inputs(M, N, E, seed):
    """O(1) features, logits of a few units."""
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(M, E, generator=g)
    W = torch.randn(N, E, generator=g) / (E ** 0.5)
    b = torch.randn(N, generator=g)
    return feat.numpy(), W.numpy(), b.numpy()


def _plants(N):
    """Equal winners: one lane's column class (3, 7), the two lane halves of a row (3, 19), sub-tiles and N tiles (35, 131), the
    edges 127 / 128, N - 1 and the ragged last tile."""
    last = N - N % 128 if N % 128 else N - 128
    return sorted({3, 7, 19, 35, 127, 128, 131, last + 2, N - 1} & set(range(N)))


def _exact_inputs(M, N, E, seed, plants, lift):
    """Features in {-2..2}, weights and biases multiples of 2^-4 in [-1/4, 1/4] ([-1, 1]): logits are multiples of 2^-4 of a few
    units, exact in fp32 in any order.  The columns of `plants` share one weight row and one bias `lift` above it: equal in every
    row, the winners -- the lowest index must be returned."""
    rng = np.random.RandomState(seed)
    feat = rng.randint(-2, 3, size=(M, E)).astype(np.float32)
    W = (rng.randint(-4, 5, size=(N, E)) / 16.0).astype(np.float32)
    b = (rng.randint(-16, 17, size=N) / 16.0).astype(np.float32)
    for c in plants[1:]:
        W[c] = W[plants[0]]
    for c in plants:
        b[c] = lift
    return feat, W, b


def _targets(M, N, seed, extra=()):
    """Random targets with every second row on an edge: column 0, N - 1, 127, 128 (the last column of a tile and the first of the
    next), the ragged tail, skipped rows (negative) and targets past the head (N, N + 1000, beyond 2^31)."""
    rng = np.random.RandomState(seed + 17)
    t = rng.randint(0, N, size=M).astype(np.int64)
    tail = N - 1 - (N % 128) // 2 if N % 128 else N - 2
    specials = [0, N - 1, min(127, N - 1), min(128, N - 1), max(tail, 0), -1, N, -(2 ** 40), N + 1000, 2 ** 40 + 5] + list(extra)
    for r in range(0, M, 2):
        t[r] = specials[(r // 2) % len(specials)]
    return t


def _case_table():
    cases = {}

    def add(kind, M, N, E, **kw):
        name = "%s-%d-%d-%d%s" % (kind, M, N, E, kw.pop("tag", ""))
        cases[name] = dict(kind=kind, M=M, N=N, E=E, **kw)

    # every (E, N) pair once; M and the kind walk along both axes (six N against five M: every (E, M) pair appears too)
    for i, E in enumerate(FUSED_E + GENERIC_E):
        for j, N in enumerate(NS):
            add("exact" if (i + j) % 2 else "random", MS[(i + j) % 5], N, E)
    # three row blocks at the widest head: 24 units, 1 to 4 workgroups on a row block at the grids of the tests
    add("exact", 257, 1000, 64, tag="-rb")
    add("random", 257, 1000, 128, tag="-rb")
    # logits spread over +-80 (the bias): an unrescaled sum overflows or vanishes
    add("spread", 131, 1000, 64)
    add("spread", 33, 300, 128)
    add("spread", 33, 300, 32)
    # -inf bias columns, on targets too
    add("masked", 131, 300, 128)
    add("masked", 33, 1000, 64)
    add("masked", 31, 129, 256)
    # even rows: maximum in the first tile, target in the last; odd rows the reverse
    add("planted", 131, 1000, 64)
    add("planted", 257, 300, 128)
    add("planted", 33, 300, 32)
    # a row pitch wider than the features
    add("random", 33, 129, 64, ldf=80, tag="-pitch")
    add("exact", 131, 300, 128, ldf=132, tag="-pitch")
    add("random", 31, 127, 32, ldf=48, tag="-pitch")
    return cases


CASES = _case_table()
REPEAT_CASES = ("exact-257-1000-64-rb", "random-257-1000-128-rb")
ROWS_CASES = {"%s-%d" % (kind, n): (kind, 37, n) for kind in ("random", "exact") for n in (1, 63, 64, 65, 1000)}


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % 100003


@functools.lru_cache(maxsize=None)
def build(name):
    """-> (feat [M, ldf], W [N, E], b [N], target [M], Ref) of a case; computed once per process, treat as read-only."""
    c = CASES[name]
    M, N, E, kind, seed = c["M"], c["N"], c["E"], c["kind"], _seed(name)
    extra = ()
    if kind == "exact":
        feat, W, b = _exact_inputs(M, N, E, seed, _plants(N), 24.0)
    elif kind == "planted":
        feat, W, b = _exact_inputs(M, N, E, seed, [], 0.0)
        first, last = 5, N - 3
        feat[0::2, 0], feat[1::2, 0] = 2.0, -2.0
        W[:, 0] = 0.0
        W[first, 0], W[last, 0] = 16.0, -16.0          # +-32 on top of logits of a few units
    else:
        feat, W, b = _random_inputs(M, N, E, seed)
        if kind == "spread":
            b = np.random.RandomState(seed).uniform(-80.0, 80.0, size=N).astype(np.float32)
        if kind == "masked":
            rng = np.random.RandomState(seed)
            masked = sorted(set(rng.choice(N, size=N // 5, replace=False).tolist()) | {0, 127, N - 1})
            b = b.copy()
            b[masked] = -np.inf
            assert np.isfinite(b).any()
            extra = (masked[1], masked[-2], masked[len(masked) // 2])
    target = _targets(M, N, seed, extra)
    if kind == "planted":
        target[0::2], target[1::2] = N - 3, 5
    ref = linear_ref(feat, W, b, target, exact_valued=kind in ("exact", "planted"))
    ldf = c.get("ldf", E)
    if ldf > E:
        feat = np.concatenate([feat, np.full((M, ldf - E), PAD, dtype=np.float32)], axis=1)
    return np.ascontiguousarray(feat), W, b, target, ref


@functools.lru_cache(maxsize=None)
def build_rows(name):
    kind, M, n = ROWS_CASES[name]
    if kind == "exact":
        rng = np.random.RandomState(n)
        x = (rng.randint(-64, 65, size=(M, n)) / 16.0).astype(np.float32)
        if n > 2:
            x[:, n - 1] = x[:, 0] = 8.0           # equal winners at both ends
    else:
        x = torch.randn(M, n, generator=torch.Generator().manual_seed(n)).numpy() * 30      # (logits over +-80 and more)
    target = _targets(M, n, n)
    return x, target, rows_ref(x, target, exact_valued=kind == "exact")
