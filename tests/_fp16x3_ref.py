"""The fp16x3 operand format restated in NumPy from its definition (include/tal_asrd.h), independent of the kernels:

    hi = fp16(x)                       round to nearest even, fp16 subnormals kept
    lo = fp16((x - hi) * 2^11)         the subtraction and the scaling in fp32 (both exact for |x| inside the fp16 range)
    value carried = hi + lo * 2^-11
    x . w ~ sum hi_x hi_w + 2^-11 sum (hi_x lo_w + lo_x hi_w)              (lo_x lo_w dropped)

Two variants exist in the kernels.  The CLAMPED one (`split_f16x3`) limits both halves to +-65504 before the conversion, so
no half is ever infinite; the PLAIN one (`split_f16x3_pair`, used under the range guard) converts as is.  What each does with
values outside the window is written out in NONFINITE_TABLE below; the GPU tests assert that table.

Byte geometry of a split row (same bytes as the fp32 row): per 32-wide K block 32 hi halves, then 32 lo halves."""
import numpy as np

F16_MAX = 65504.0
LO_SCALE = 2048.0
F16_MIN_NORMAL = 2.0 ** -14
F16_MIN_SUBNORMAL = 2.0 ** -24


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def split_plain(x):
    """(hi, lo) float16 arrays of the unclamped split: what a guarded kernel stores."""
    x = _f32(x)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(np.float16)
        lo = ((x - hi.astype(np.float32)) * np.float32(LO_SCALE)).astype(np.float16)
    return hi, lo


def _clamp_like_kernel(x):
    """fminf(fmaxf(x, -65504), 65504): IEEE maxNum / minNum return the other operand for a NaN, so NaN -> -65504."""
    x = _f32(x)
    with np.errstate(invalid="ignore"):
        y = np.fmin(np.fmax(x, np.float32(-F16_MAX)), np.float32(F16_MAX))
    return y.astype(np.float32)


def split_clamped(x):
    """(hi, lo) of the clamped split (tal_split_f16x3_fwd and every unguarded converting site)."""
    x = _f32(x)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = _clamp_like_kernel(x).astype(np.float16)
        lo = _clamp_like_kernel((x - hi.astype(np.float32)) * np.float32(LO_SCALE)).astype(np.float16)
    return hi, lo


def decode(hi, lo):
    """float64 value a (hi, lo) pair stands for."""
    return np.asarray(hi, dtype=np.float64) + np.asarray(lo, dtype=np.float64) / LO_SCALE


def pack_rows(hi, lo):
    """[rows, K] halves -> the bytes of the split form as uint16 [rows, K / 32, 64] (32 hi, then 32 lo per block)."""
    hi = np.asarray(hi, dtype=np.float16)
    lo = np.asarray(lo, dtype=np.float16)
    rows, K = hi.shape
    assert K % 32 == 0
    out = np.empty((rows, K // 32, 64), dtype=np.uint16)
    out[:, :, :32] = hi.view(np.uint16).reshape(rows, K // 32, 32)
    out[:, :, 32:] = lo.view(np.uint16).reshape(rows, K // 32, 32)
    return out


def unpack_rows(buf_u16, rows, K):
    """inverse of pack_rows: uint16 words of a split buffer -> (hi, lo) float16 [rows, K]."""
    b = np.asarray(buf_u16, dtype=np.uint16).reshape(rows, K // 32, 64)
    hi = np.ascontiguousarray(b[:, :, :32]).reshape(rows, K).view(np.float16)
    lo = np.ascontiguousarray(b[:, :, 32:]).reshape(rows, K).view(np.float16)
    return hi, lo


def decode_rows(buf_u16, rows, K):
    hi, lo = unpack_rows(buf_u16, rows, K)
    return decode(hi, lo)


def product_f16x3(x, w, clamped=True):
    """x [M, K] . w [N, K]^T as the format defines it, every sum in float64: what a kernel computes when only the format errs."""
    sp = split_clamped if clamped else split_plain
    hx, lx = (a.astype(np.float64) for a in sp(x))
    hw, lw = (a.astype(np.float64) for a in sp(w))
    return hx @ hw.T + (hx @ lw.T + lx @ hw.T) / LO_SCALE


def out_of_range(x):
    """the guard's predicate: True where a value must raise the status word (beyond 65504 in magnitude, or not finite)."""
    x = _f32(x)
    with np.errstate(invalid="ignore"):
        return ~(np.abs(x) <= np.float32(F16_MAX))


def interesting_f32_patterns():
    """Every fp32 pattern the conversions can get wrong, as one float32 vector whose length is a multiple of 32: +-0, fp32
    subnormals, 2^-25 .. 2^-13 densely (fp16 subnormal range and its two borders), all fp16 rounding midpoints near 1 and near
    65504 with their fp32 neighbours, 65504 .. 65536, +-Inf, NaN."""
    parts = [np.array([0.0, -0.0], dtype=np.float32)]
    sub = np.array([1, 2, 3, 0x1234, 0x400000, 0x7FFFFF], dtype=np.uint32)                   # fp32 subnormals
    parts.append(sub.view(np.float32))
    parts.append((sub | np.uint32(0x80000000)).view(np.float32))
    parts.append(np.array([2.0 ** -149, 2.0 ** -126, 2.0 ** -60, 2.0 ** -40, 2.0 ** -30, 2.0 ** -26], dtype=np.float32))
    lo_bits = np.float32(2.0 ** -25).view(np.uint32)
    hi_bits = np.float32(2.0 ** -13).view(np.uint32)
    dense = np.linspace(int(lo_bits), int(hi_bits), 6000).astype(np.uint32).view(np.float32)      # 12 binades, ~500 points each
    parts.append(dense)
    k = np.arange(0, 2049, dtype=np.float64)
    sub_mid = ((k + 0.5) * 2.0 ** -24).astype(np.float32)                                         # midpoints of the subnormal grid
    parts += [sub_mid, np.nextafter(sub_mid, np.float32(0)), np.nextafter(sub_mid, np.float32(1))]

    def midpoints(lo_h, hi_h):
        h = np.arange(np.float16(lo_h).view(np.uint16), np.float16(hi_h).view(np.uint16) + 1, dtype=np.uint16).view(np.float16)
        m = ((h[:-1].astype(np.float64) + h[1:].astype(np.float64)) / 2).astype(np.float32)          # exact in fp32
        return [h.astype(np.float32), m, np.nextafter(m, np.float32(0)), np.nextafter(m, np.float32(1e9))]
    parts += midpoints(0.97, 1.03)
    parts += midpoints(65000.0, 65504.0)
    top = np.arange(65504.0, 65537.0, 1.0, dtype=np.float32)
    parts += [top, np.nextafter(np.float32(65504.0), np.float32(1e9)).reshape(1), np.nextafter(np.float32(65520.0), np.float32(0)).reshape(1),
              np.array([65519.996, 65520.0, 7.0e4, 1.0e5, 3.0e38], dtype=np.float32)]
    parts.append(np.array([np.inf, -np.inf, np.nan], dtype=np.float32))
    v = np.concatenate([p.astype(np.float32).ravel() for p in parts])
    v = np.concatenate([v, -v])
    pad = (-v.size) % 32
    return np.concatenate([v, np.ones(pad, dtype=np.float32)])


# What the two variants make of a value outside the window: (x, clamped (hi, lo), plain (hi, lo), guard fires).  NaN halves are
# written as the string "nan".  65505 .. 65519.99 round to 65504 in fp16 and are still out of range; 65520 rounds to Inf.
NONFINITE_TABLE = [
    # x           clamped hi, lo                 plain hi, lo                   guard
    (65504.0,     (65504.0, 0.0),                (65504.0, 0.0),                False),
    (65505.0,     (65504.0, 2048.0),             (65504.0, 2048.0),             True),
    (65519.0,     (65504.0, 30720.0),            (65504.0, 30720.0),            True),
    (65520.0,     (65504.0, 32768.0),            (np.inf, -np.inf),             True),
    (1.0e5,       (65504.0, 65504.0),            (np.inf, -np.inf),             True),
    (-1.0e5,      (-65504.0, -65504.0),          (-np.inf, np.inf),             True),
    (np.inf,      (65504.0, 65504.0),            (np.inf, "nan"),               True),
    (-np.inf,     (-65504.0, -65504.0),          (-np.inf, "nan"),              True),
    (np.nan,      (-65504.0, -65504.0),          ("nan", "nan"),                True),
]


# ---------------------------------------------------------------------------------------------------------------------
# Seeded inputs of the head tests (shared by the CPU check of the skip condition and the GPU tests)
HEAD_M, HEAD_E, HEAD_S = 3000, 128, 6008       # the smallest row count that takes the long-input arg-max form at S = 6008
SWEEP_EXPONENTS = (-40, -30, -24, -20, -14, -8, 0, 8, 14)
RANDN_CLIP = 3.9                                # 3.9 * 2^14 = 63898 <= 65504: the top sweep entries stay inside the window


def clipped_randn(rng, shape):
    return np.clip(rng.standard_normal(shape), -RANDN_CLIP, RANDN_CLIP).astype(np.float32)


def head_case(p, seed=5):
    """features [M, 128] * 2^p, logit weight [S, 128] / 11, logit bias [S]: float32 arrays."""
    rng = np.random.default_rng(seed)
    feat = (clipped_randn(rng, (HEAD_M, HEAD_E)) * np.float32(2.0 ** p)).astype(np.float32)
    wl = (rng.standard_normal((HEAD_S, HEAD_E)) / 11).astype(np.float32)
    bl = rng.standard_normal(HEAD_S).astype(np.float32)
    return feat, wl, bl


def head_reference(feat, wl, bl):
    """float64 logits, their arg-max, and the rows the margin rule keeps: top-2 margin > 8 * e32, e32 = the largest error of
    that ROW's logits computed in float32 on the host against float64 (per row: one huge row must not excuse the others).
    A NaN logit never wins in any arg-max of the library (`v > best`), so it counts as -inf here; +-Inf logits take part as
    they are.  A row without a finite-or-infinite winner (all NaN) is not kept.  Returns (logits, argmax, keep, max e32)."""
    with np.errstate(invalid="ignore", over="ignore"):
        want = feat.astype(np.float64) @ wl.astype(np.float64).T + bl.astype(np.float64)
        got32 = (feat @ wl.T + bl).astype(np.float64)
        d = np.abs(got32 - want)
        e32 = np.where(np.isfinite(d), d, 0.0).max(axis=1)
        ranked = np.where(np.isnan(want), -np.inf, want)
        top2 = np.partition(ranked, -2, axis=1)[:, -2:]
        margin = top2[:, 1] - top2[:, 0]                    # inf - finite = inf (kept); -inf - -inf = NaN (not kept)
        keep = margin > 8 * e32
    return want, np.argmax(ranked, axis=1), keep, float(e32.max())
