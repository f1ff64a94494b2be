"""Float64 model of the softmax-weighted embeddings (tal_soft_embed_fwd, tal_soft_embed_rows, tal_lm_soft_embed_fwd), the case table the
CPU and GPU tests share, and the comparison with its error bound.

Semantics (include/tal_asrd.h): z[r, s] = feat[r, :] . W[s, :] + b[s], lse[r] = log sum_s exp(z[r, s]),
out[r, :] = sum_s exp(z[r, s] - lse[r]) values[s, :] (values None: values = W).  A -inf bias masks a column: nothing in lse or out.

Error bound of out[r, d], u = 2^-24, gamma_n = n u / (1 - n u), p = the exact softmax of the row, A[r, d] = sum_s p_s |values[s, d]|,
a_s = z_s - max_s z_s <= 0.  Every term is derived, none is fitted:
  (1) logit rounding.  B[r, s] = gamma_{E+2} (sum_k |feat[r, k]| |W[s, k]| + |b[s]|) bounds an fp32 logit (E products, E - 1 additions,
      the bias) in any order of summation; Bmax = max_s B[r, s] (with the gamma of tests/_head_topk_ref.py).  Logits off by at most
      Bmax move every p_s by a factor within exp(+-2 Bmax) (numerator and normaliser one Bmax each): 2 Bmax in the exponent R below.
  (2) the exp argument and result.  The subtraction z_s - m rounds once (|a_s| u); the fast exponential multiplies by an fp32 log2(e)
      (the constant's rounding and the product's: 2 |a_s| u) and returns 2^x within 2 u: eps_s = (3 |a_s| + 2) u relative to each
      exponential.  They do not cancel between terms: the numerator moves by NE[r, d] = sum_s p_s eps_s |values[s, d]|, the normaliser
      by SE[r] = sum_s p_s eps_s (into R).  (The rescale factors exp(m_old - m_new) of the online form and of the merge multiply the
      running sum and the output accumulators alike: their own error cancels in the quotient, only their roundings count, in (3) / (5).)
  (3) accumulation over N, weighted by A: N products and N - 1 additions of the numerator in any order, and at most one further
      rounding per column from rescaling the accumulators (a rescale happens at most once per tile of columns): gamma_{2N + 2} A;
      the normaliser's N additions and rescales likewise: another gamma_{2N + 2} in R.
  (4) normalisation: one division (the fused form: of the sum; the generic form: of every probability, before the product): 2 u in R.
  (5) the merge of at most 16 partials per row: one product and one addition each, numerator and normaliser: 2 gamma_32 in R.
  (6) exponentials below the normal range (a_s < -87) are flushed: at most 2^-126 absolute per term, N 2^-126 max |values| in all.
  R = 2 Bmax + SE + 2 gamma_{2N + 2} + 2 u + 2 gamma_32;   |out - exact| <= expm1(R) A + (1 + R) NE + N 2^-126 max |values|.
lse: as tests/_xent_ref.py, |lse - exact| <= Bmax + (N + 64) u + 2 u |lse|.

Exact-valued cases (small-integer features and values, weights and biases multiples of 2^-4, winners at least 120 above every other
logit so that every other exponential is 0.0f) must come out BIT-EQUAL to the model: values[winner], or the exact mean of 2 / 4 winners.
"""
import functools

import numpy as np
import torch

from tests._head_topk_ref import gamma

U = 2.0 ** -24
TILE = 64                   # columns per step of the online variants below (a model of "some tiling", not the kernel's constant)

VARIANTS = ("values_row_off_by_one", "keys_as_values", "bias_left_out", "masked_column_counted", "merge_without_rescale",
            "accumulator_not_rescaled", "last_tile_sum_only")

FUSED_WIDTHS = (128, 64)    # (E, D) = (w, w) has a fused form
NS = (1, 127, 128, 129, 300)
MS = (1, 33, 129)
PAD = 777.0                 # what the columns behind a row's E features hold when ldf > E
LIFT = 200.0                # bias of a planted winner: >= 120 above every other logit (asserted in build)


# ------------------------------------------------------------------ the model
def _softmax(z):
    m = z.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.exp(z - m)
    s = e.sum(axis=1, keepdims=True)
    return e / s, (m + np.log(s))[:, 0]


def _online(z, V, rescale_acc=True, last_sum_only=False):
    """The online form over tiles of TILE columns: running (max, sum, acc)."""
    M, N = z.shape
    m = np.full(M, -np.inf)
    s = np.zeros(M)
    acc = np.zeros((M, V.shape[1]))
    last = s
    for c0 in range(0, N, TILE):
        zt = z[:, c0:c0 + TILE]
        mn = np.maximum(m, zt.max(axis=1))
        ms = np.where(np.isfinite(mn), mn, 0.0)
        with np.errstate(invalid="ignore"):
            f = np.where(np.isfinite(m), np.exp(m - ms), 0.0)
            p = np.exp(zt - ms[:, None])
        last = p.sum(axis=1)
        s = s * f + last
        acc = (acc * f[:, None] if rescale_acc else acc) + p @ V[c0:c0 + TILE]
        m = mn
    with np.errstate(invalid="ignore", divide="ignore"):
        return acc / (last if last_sum_only else s)[:, None], m + np.log(s)


def soft_embed(zr, b, W, V, variant=None):
    """zr [M, N] float64 = feat . W^T, b [N] float64 (may hold -inf), W [N, E], V [N, D] float64 -> out [M, D], lse [M].
    variant: one of VARIANTS, a plausible wrong kernel."""
    z = zr + b
    if variant == "bias_left_out":
        z = zr
    elif variant == "masked_column_counted":
        z = zr + np.where(np.isfinite(b), b, 0.0)
    if variant == "values_row_off_by_one":
        V = np.roll(V, 1, axis=0)
    elif variant == "keys_as_values":
        V = W
    if variant == "accumulator_not_rescaled":
        return _online(z, V, rescale_acc=False)
    if variant == "last_tile_sum_only":
        return _online(z, V, last_sum_only=True)
    if variant == "merge_without_rescale" and z.shape[1] > 1:
        # two partials (max, sum, acc) of the two halves of the columns, added as they are under the larger maximum
        h = z.shape[1] // 2
        parts = []
        for zs, Vs in ((z[:, :h], V[:h]), (z[:, h:], V[h:])):
            m = zs.max(axis=1)
            ms = np.where(np.isfinite(m), m, 0.0)
            e = np.exp(zs - ms[:, None])
            parts.append((m, e.sum(axis=1), e @ Vs))
        s = parts[0][1] + parts[1][1]
        with np.errstate(invalid="ignore"):
            return (parts[0][2] + parts[1][2]) / s[:, None], np.maximum(parts[0][0], parts[1][0]) + np.log(s)
    p, lse = _softmax(z)
    return p @ V, lse


class Ref:
    """The exact results of a case and what `compare` needs."""

    def __init__(self, zr, b, B, W, V, exact_valued, separate):
        self.zr, self.b, self.W, self.V, self.exact_valued, self.separate = zr, b, W, V, exact_valued, separate
        z = zr + b
        self.z = z
        self.M, self.N = z.shape
        self.D = V.shape[1]
        self.out, self.lse = soft_embed(zr, b, W, V)
        p, _ = _softmax(z)
        absV = np.abs(V)
        self.Bmax = np.where(np.isfinite(z), B, 0.0).max(axis=1)                                  # (1)
        with np.errstate(invalid="ignore"):
            a = np.where(np.isfinite(z), z - z.max(axis=1, keepdims=True), 0.0)
        eps = (3.0 * np.abs(a) + 2.0) * U                                                         # (2)
        A = p @ absV
        NE = (p * eps) @ absV
        SE = (p * eps).sum(axis=1)
        R = 2 * self.Bmax + SE + 2 * gamma(2 * self.N + 2) + 2 * U + 2 * gamma(32)                # (1) (2) (3) (4) (5)
        self.tol = np.expm1(R)[:, None] * A + (1 + R)[:, None] * NE + self.N * 2.0 ** -126 * absV.max()      # ... (6)
        self.lse_tol = self.Bmax + (self.N + 64) * U + 2 * U * np.abs(self.lse)

    def wrong(self, variant):
        return soft_embed(self.zr, self.b, self.W, self.V, variant=variant)


def make_ref(feat, W, b, values, exact_valued=False):
    """feat [M, E] (the features alone, without the padding of a pitched row); values None: values = W."""
    f, w = feat.astype(np.float64), W.astype(np.float64)
    bb = np.zeros(W.shape[0]) if b is None else b.astype(np.float64)
    B = gamma(feat.shape[1] + 2) * (np.abs(f) @ np.abs(w).T + np.where(np.isfinite(bb), np.abs(bb), 0.0))
    return Ref(f @ w.T, bb, B, w, w if values is None else values.astype(np.float64), exact_valued, values is not None)


def rows_ref(x, values, exact_valued=False):
    """tal_soft_embed_rows: the matrix is given, so nothing rounds in front of the exponentials' argument (B = 0)."""
    x64 = x.astype(np.float64)
    return Ref(x64, np.zeros(x.shape[1]), np.zeros(x.shape), values.astype(np.float64), values.astype(np.float64), exact_valued, True)


def error_ratio(ref, out):
    """largest |out - exact| / bound over the case (0 where both vanish)"""
    err = np.abs(np.asarray(out, dtype=np.float64) - ref.out)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.where(err == 0.0, 0.0, err / ref.tol)))


def compare(ref, out, lse=None):
    """-> list of messages, empty when (out [M, D], lse [M] or None) is within the bound of the model (bit-equal for exact cases)."""
    out = np.asarray(out)
    bad = []
    if out.shape != (ref.M, ref.D) or (lse is not None and np.asarray(lse).shape != (ref.M,)):
        return ["shapes %s %s" % (out.shape, None if lse is None else np.asarray(lse).shape)]
    if ref.exact_valued:
        want = ref.out.astype(np.float32)
        assert np.array_equal(want.astype(np.float64), ref.out), "the case is not exact-valued"
        with np.errstate(over="ignore"):
            got = out.astype(np.float32)
        if not np.array_equal(got.view(np.int32), want.view(np.int32)):
            r, d = np.argwhere(got.view(np.int32) != want.view(np.int32))[0]
            bad.append("out[%d, %d] is not bit-equal: %r vs %r (%d elements)" % (r, d, got[r, d], want[r, d],
                                                                                (got.view(np.int32) != want.view(np.int32)).sum()))
    err = np.abs(out.astype(np.float64) - ref.out)
    ok = err <= ref.tol                 # (NaN fails)
    if not ok.all():
        r, d = np.argwhere(~ok)[0]
        bad.append("out[%d, %d]: %r vs %r (bound %.3e, %d elements)" % (r, d, out[r, d], ref.out[r, d], ref.tol[r, d], (~ok).sum()))
    if lse is not None:
        lerr = np.abs(np.asarray(lse, dtype=np.float64) - ref.lse)
        if not np.all(lerr <= ref.lse_tol):
            r = int(np.argmax(np.where(np.isnan(lerr), np.inf, lerr - ref.lse_tol)))
            bad.append("lse row %d: %r vs %r (bound %.3e)" % (r, lse[r], ref.lse[r], ref.lse_tol[r]))
    return bad


# ------------------------------------------------------------------ the cases
def _random_inputs(M, N, E, D, seed):
    """O(1) features, logits of a few units, asymmetric values."""
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(M, E, generator=g)
    W = torch.randn(N, E, generator=g) / (E ** 0.5)
    b = torch.randn(N, generator=g)
    V = torch.randn(N, D, generator=g) + torch.arange(D, dtype=torch.float32) / D       # (no symmetry between rows and columns)
    return feat.numpy(), W.numpy(), b.numpy(), V.numpy()


def _exact_inputs(M, N, E, D, seed, plants):
    """Features in {-2..2}, weights multiples of 2^-4 in [-1/4, 1/4], biases in [-1, 1], values integers in [-8, 8]: logits are
    multiples of 2^-4 of a few units, exact in fp32 in any order.  The columns of `plants` share one weight row and the bias LIFT:
    equal in every row and far above the rest, the winners.  Their rows of values differ."""
    rng = np.random.RandomState(seed)
    feat = rng.randint(-2, 3, size=(M, E)).astype(np.float32)
    W = (rng.randint(-4, 5, size=(N, E)) / 16.0).astype(np.float32)
    b = (rng.randint(-16, 17, size=N) / 16.0).astype(np.float32)
    V = rng.randint(-8, 9, size=(N, D)).astype(np.float32)
    for c in plants[1:]:
        W[c] = W[plants[0]]
    for c in plants:
        b[c] = LIFT
    return feat, W, b, V


def _order_inputs(M, N, E, D, seed, order):
    """The running maximum's order.  rising / falling / middle: an exact-valued head of a few units plus a bias ramp of 1 per column
    (every tile raises the maximum / only the first does / the tiles up to the middle do).  rowdep: row r's maximum at column
    (37 r) mod N through a planar rotation in the first two features (z = 40 cos(theta_r - phi_s) + a small random rest), so the rows
    of one 32-row block change their maximum at different tiles."""
    rng = np.random.RandomState(seed)
    if order == "rowdep":
        feat = (rng.randn(M, E) * 0.01).astype(np.float32)
        W = (rng.randn(N, E) * 0.01).astype(np.float32)
        th = 2 * np.pi * ((37 * np.arange(M)) % N) / N
        ph = 2 * np.pi * np.arange(N) / N
        feat[:, 0], feat[:, 1] = 40 * np.cos(th), 40 * np.sin(th)
        W[:, 0], W[:, 1] = np.cos(ph), np.sin(ph)
        b = np.zeros(N, dtype=np.float32)
    else:
        feat = rng.randint(-1, 2, size=(M, E)).astype(np.float32)
        W = (rng.randint(-2, 3, size=(N, E)) / 16.0).astype(np.float32)
        s = np.arange(N, dtype=np.float32)
        b = {"rising": s, "falling": -s, "middle": -np.abs(s - N // 2)}[order].astype(np.float32)
    V = (rng.randn(N, D) + np.arange(D) / D).astype(np.float32)
    return feat, W, b, V


def _case_table():
    cases = {}

    def add(kind, M, N, E, D=None, **kw):
        D = E if D is None else D
        name = "%s-%d-%d-%d%s" % (kind, M, N, E, kw.pop("tag", ""))
        assert name not in cases
        cases[name] = dict(kind=kind, M=M, N=N, E=E, D=D, **kw)

    # every (width, N) pair once, M walks along
    for i, E in enumerate(FUSED_WIDTHS):
        for j, N in enumerate(NS):
            add("random", MS[(i + j) % 3], N, E)
    add("random", 160, 6008, 128)                        # the speaker head: 94 tiles, several workgroups on a row block
    add("random", 33, 301, 128, tag="-n301")             # N % 4 != 0: the padded probability pitch of the generic form
    add("random", 33, 300, 32, D=20)                     # widths only the generic form takes
    add("random", 33, 129, 128, ldf=132, tag="-pitch")   # a row pitch wider than the features
    add("random", 129, 300, 64, ldf=80, tag="-pitch")
    # one planted winner: the first and last column of a tile, N - 1, inside the ragged last tile
    for col in (0, 127, 128, 290, 299):
        add("exact", 33, 300, 128, plants=(col,), tag="-w%d" % col)
    add("exact", 129, 300, 64, plants=(128,), tag="-w128")
    add("exact", 33, 129, 64, plants=(128,), tag="-w128")
    # equal winners in different tiles: the exact mean
    add("exact", 33, 300, 128, plants=(5, 200), tag="-two")
    add("exact", 129, 300, 128, plants=(3, 70, 130, 297), tag="-four")
    add("exact", 129, 300, 64, plants=(63, 64, 191, 299), tag="-four")
    add("exact", 33, 301, 32, D=20, plants=(3, 300), tag="-two")
    # the order of the running maximum
    for order in ("rising", "falling", "middle", "rowdep"):
        add("order", 129, 300, 128, order=order, tag="-" + order)
    add("order", 129, 300, 64, order="rising", tag="-rising")
    add("order", 129, 300, 64, order="rowdep", tag="-rowdep")
    # -inf bias: the whole first 128 columns (the running maximum is still -inf when the first finite tile arrives), scattered
    add("masked", 33, 300, 128, mask="first", tag="-first")
    add("masked", 129, 300, 64, mask="first", tag="-first")
    add("masked", 129, 300, 128, mask="scattered", tag="-scattered")
    add("masked", 33, 129, 64, mask="scattered", tag="-scattered")
    return cases


CASES = _case_table()
REPEAT_CASES = ("random-160-6008-128", "order-129-300-64-rowdep")
ROWS_CASES = {"%s-%d" % (kind, n): (kind, 37, n) for kind in ("random", "exact") for n in NS + (301,)}


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % 100003


@functools.lru_cache(maxsize=None)
def build(name):
    """-> (feat [M, ldf], W [N, E], b [N], values [N, D], ref with values = W or None, ref with `values`) of a case; computed once
    per process, treat as read-only."""
    c = CASES[name]
    M, N, E, D, kind, seed = c["M"], c["N"], c["E"], c["D"], c["kind"], _seed(name)
    if kind == "exact":
        feat, W, b, V = _exact_inputs(M, N, E, D, seed, list(c["plants"]))
    elif kind == "order":
        feat, W, b, V = _order_inputs(M, N, E, D, seed, c["order"])
    else:
        feat, W, b, V = _random_inputs(M, N, E, D, seed)
        if kind == "masked":
            rng = np.random.RandomState(seed)
            masked = list(range(min(128, N - 1))) if c["mask"] == "first" else \
                sorted(set(rng.choice(N, size=N // 5, replace=False).tolist()) | {0, 63, 64, 127, N - 1})
            b = b.copy()
            b[masked] = -np.inf
            assert np.isfinite(b).any()
    exact = kind == "exact"
    ref_alias = make_ref(feat, W, b, None, exact) if D == E else None
    ref_sep = make_ref(feat, W, b, V, exact)
    if exact:
        z = ref_sep.z
        win = list(c["plants"])
        rest = np.delete(z, win, axis=1)
        assert (z[:, win].min(axis=1) == z[:, win].max(axis=1)).all()
        assert rest.size == 0 or (z[:, win[0]] - rest.max(axis=1)).min() >= 120.0
        # every other exponential is below exp(-120) = 8e-53 of a winner's: 0.0f in fp32 (the smallest subnormal is 1.4e-45), so
        # what an fp32 evaluation must give is the winners' mean itself; the float64 model agrees with it to ~1e-50
        for ref, vals in ((ref_alias, W), (ref_sep, V)):
            if ref is not None:
                mean = vals[win].astype(np.float64).mean(axis=0)[None].repeat(M, axis=0)
                assert np.abs(ref.out - mean).max() < 1e-45
                ref.out = mean
    ldf = c.get("ldf", E)
    if ldf > E:
        feat = np.concatenate([feat, np.full((M, ldf - E), PAD, dtype=np.float32)], axis=1)
    return np.ascontiguousarray(feat), W, b, V, ref_alias, ref_sep


@functools.lru_cache(maxsize=None)
def build_rows(name):
    """-> (x [37, n], values [n, 24], ref) of a materialised matrix"""
    kind, M, n = ROWS_CASES[name]
    rng = np.random.RandomState(n)
    if kind == "exact":
        x = (rng.randint(-64, 65, size=(M, n)) / 16.0).astype(np.float32)
        x[:, n - 1] = x[:, 0] = 150.0             # equal winners at both ends (one winner at n = 1)
        V = rng.randint(-8, 9, size=(n, 24)).astype(np.float32)
    else:
        x = (torch.randn(M, n, generator=torch.Generator().manual_seed(n)).numpy() * 30).astype(np.float32)   # (logits over +-80 and more)
        V = (rng.randn(n, 24) + np.arange(24) / 24).astype(np.float32)
    return x, V, rows_ref(x, V, exact_valued=kind == "exact")
