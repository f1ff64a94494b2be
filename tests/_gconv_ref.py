"""The grouped temporal convolutions of csrc/gconv.hip and csrc/gconv_general.hip as an exact model, the banded buffers the GPU
test hands to the C entry points, and the table of cases.  Nothing here calls the library.

Model (tal/asr/models.py:363-364 and :304-308,329): torch.nn.functional.conv1d in float64 on [B, C, T] --
  stride 2, padding 0                               the resize convs,
  x + alpha * relu(conv(x, padding=k // 2) + b)     the TDSBlock convs --
returned in the kernels' time-major [B, T, C]; `reference_loops` restates it as three numpy loops for tiny cases.

Exact data.  x holds integers in [-8, 8], w integers in [-4, 4]; block convs take an integer bias in [-16, 16] and alpha = 2^-10,
resize convs a bias in multiples of 1/16 with |b| <= 16.  Then every operand is one fp16 half (its lo half is 0), every partial
sum has at most 18 significant bits in whatever order it is taken (k = 21: below 18 * 21 * 32 + 16 = 12112, 14 integer bits and
the 4 fractional bits of the bias; k = 63: below 36304 with an integer bias), and every output is exact in fp32 and in the 22-bit
hi / lo split form.  So the comparison is EQUALITY, and a wrong element names its (item, step, channel).
tests/test_gconv_ref_cpu.py asserts these premises on the data of every case.  The lo halves of the INPUTS are zero by construction:
the hi * lo product terms of the fp16x3 kernels are checked by the tolerance tests on random data (tests/test_gpu_parity.py,
tests/test_gpu_stress.py), not here; the lo halves of the OUTPUTS are non-zero for a quarter to a third of the elements (1.5 % for
the 1 -> 10 conv), so a kernel that drops or garbles them is seen.

Buffers.  Every input of a call sits inside one allocation with poison around it: x as [32 rows | x | 288 rows] with quiet NaNs
in the bands (split form: bytes 0x7E, NaN halves), bias / packed weights / fragments followed by a NaN band, payloads 16-byte
aligned.  Every output sits in [32 rows | payload | 288 rows] of bytes 0x5A.  288 rows are the longest tile with its halo
(255 + 21 input rows, 256 output rows) and one more 16-row block: a store that runs one block or one tile past the end lands in
the band, not outside the allocation.  `check` wants both bands byte-identical to the fill, every payload element finite and the
payload equal to the model (fp32 by value, the split form as hi + lo / 2048).

MUTANTS are the plausible wrong kernels; tests/test_gconv_ref_cpu.py shows that `check` rejects each on a case of the table."""
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

FRONT, BACK = 32, 288           # band rows in front of / behind x and every output
FILL = 0x5A                     # output fill
AUX_BAND = 4096                 # NaN bytes behind bias / weights / fragments
ALPHA = 2.0 ** -10
OPTION_DEFAULTS = {"gconv_short_below": 4, "gconv_long_tt": 0, "gconv_grid_xyz": 0, "gconv_no_shift18": 0, "gconv_c1_generic": 0}

# one conv problem: x [B, T, G * cig] -> [B, T_out, G * cog]
Key = namedtuple("Key", "stride cig cog G k B T")
# entry: a row of ENTRIES; opts: ((option, value), ...) in force during the call; same: cases with the same value are forms the project
# calls bit-identical (tile lengths, grid order, any-k kernel at k = 21)
Case = namedtuple("Case", "name entry key opts same")

# entry -> (C function, x in the split form, output forms)
ENTRIES = {
    "res": ("tal_gconv_res_fwd", False, ("f32",)),
    "s2": ("tal_gconv_s2_fwd", False, ("f32",)),
    "res_k": ("tal_gconv_res_k_fwd", False, ("f32",)),
    "s2_k": ("tal_gconv_s2_k_fwd", False, ("f32",)),
    "res_f16x3": ("tal_gconv_res_f16x3_fwd", False, ("f32",)),
    "res_f16x3_ys": ("tal_gconv_res_f16x3_fwd", False, ("f32", "split")),
    "s2_f16x3": ("tal_gconv_s2_f16x3_fwd", False, ("f32",)),
    "res_split": ("tal_gconv_res_split_fwd", True, ("split",)),
    "s2_split": ("tal_gconv_s2_split_fwd", True, ("split",)),
    "s2_split_f32in": ("tal_gconv_s2_split_fwd", False, ("split",)),
}
MFMA_ENTRIES = ("res_f16x3", "res_f16x3_ys", "s2_f16x3", "res_split", "s2_split", "s2_split_f32in")


def out_len(key):
    return key.T if key.stride == 1 else (key.T - key.k) // 2 + 1


def channels(key):
    return key.G * key.cig, key.G * key.cog


def _rng(*what):
    return np.random.RandomState(zlib.crc32(repr(what).encode()))


# ------------------------------------------------------------------------------------------------------------------
# data and model
# ------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def weights(stride, cig, cog, G, k):
    """(w [G * cog, cig, k] in the reference's Conv1d layout, bias [G * cog]) as float64; shared by every T and B."""
    rng = _rng("w", stride, cig, cog, G, k)
    w = rng.randint(-4, 5, size=(G * cog, cig, k)).astype(np.float64)
    if stride == 1:
        b = rng.randint(-16, 17, size=G * cog).astype(np.float64)
    else:
        b = rng.randint(-256, 257, size=G * cog) / 16.0
    w.setflags(write=False), b.setflags(write=False)
    return w, b


@lru_cache(maxsize=24)
def x_of(key):
    x = _rng("x", *key).randint(-8, 9, size=(key.B, key.T, key.G * key.cig)).astype(np.float32)
    x.setflags(write=False)
    return x


def pack_weight(w, G):
    """[C_out, cig, k] -> the packed layout [G][cig][k][cog] of tal_pack_gconv_weight, fp32."""
    c_out, cig, k = w.shape
    return np.ascontiguousarray(w.reshape(G, c_out // G, cig, k).transpose(0, 2, 3, 1)).astype(np.float32)


def reference(x, w, b, stride, G, alpha=ALPHA):
    """The float64 model: x [B, T, C_in] -> [B, T_out, C_out]."""
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64)).permute(0, 2, 1)
    wt, bt = torch.from_numpy(np.array(w, dtype=np.float64)), torch.from_numpy(np.array(b, dtype=np.float64))
    if stride == 2:
        y = torch.nn.functional.conv1d(xt, wt, bt, stride=2, padding=0, groups=G)
    else:
        y = xt + alpha * torch.relu(torch.nn.functional.conv1d(xt, wt, bt, padding=w.shape[-1] // 2, groups=G))
    return y.permute(0, 2, 1).contiguous().numpy()


def reference_loops(x, w, b, stride, G, alpha=ALPHA):
    """The same statement as loops over output element, input channel and tap (tiny cases only)."""
    x, w, b = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64), np.asarray(b, dtype=np.float64)
    B, T, c_in = x.shape
    c_out, cig, k = w.shape
    cog = c_out // G
    pad = k // 2 if stride == 1 else 0
    t_out = T if stride == 1 else (T - k) // 2 + 1
    y = np.zeros((B, t_out, c_out))
    for bi in range(B):
        for t in range(t_out):
            for c in range(c_out):
                g = c // cog
                acc = b[c]
                for ci in range(cig):
                    for j in range(k):
                        ti = t * stride - pad + j
                        if 0 <= ti < T:
                            acc += w[c, ci, j] * x[bi, ti, g * cig + ci]
                y[bi, t, c] = acc if stride == 2 else x[bi, t, c] + alpha * max(acc, 0.0)
    return y


@lru_cache(maxsize=12)
def model(key):
    """What a perfect kernel returns for the case's data: float64 [B, T_out, C_out] (shared: do not write to it)."""
    w, b = weights(key.stride, key.cig, key.cog, key.G, key.k)
    y = reference(x_of(key), w, b, key.stride, key.G)
    y.setflags(write=False)
    return y


def wrong_model(key, flip=False, shift=0, ends="zeros", s2_off=0, relu=True, res_shift=0):
    """The model with one rule broken.  flip: taps reversed.  shift: padding k // 2 + shift (stride 1).  ends: what lies outside an
    item -- "zeros"; "neighbour": the flat [B * T] buffer, i.e. the previous item's tail and the next item's head (zeros around the
    whole); "poison": the same with NaN around the whole, the bands of the GPU test.  s2_off: stride-2 windows start at 2 t + s2_off.
    relu: False leaves it out.  res_shift: the residual comes from row t + res_shift."""
    w, b = weights(key.stride, key.cig, key.cog, key.G, key.k)
    x = x_of(key).astype(np.float64)
    B, T, c_in = x.shape
    k, t_out = key.k, out_len(key)
    if flip:
        w = w[:, :, ::-1].copy()
    left = k // 2 + shift if key.stride == 1 else -s2_off
    need = (t_out - 1) * key.stride + k              # rows a whole item reads, from row -left on
    P = need + abs(left) + 2
    flat = x.reshape(B * T, c_in)
    around = np.full((P, c_in), np.nan if ends == "poison" else 0.0)
    big = np.concatenate([around, flat, around])
    wt, bt = torch.from_numpy(w.copy()), torch.from_numpy(b.copy())
    out = np.empty((B, t_out, key.G * key.cog))
    for bi in range(B):
        if ends == "zeros":
            item = np.concatenate([np.zeros((P, c_in)), x[bi], np.zeros((P, c_in))])
            slab = item[P - left:P - left + need]
        else:
            slab = big[P + bi * T - left:P + bi * T - left + need]
        xt = torch.from_numpy(np.ascontiguousarray(slab.T))[None]
        conv = torch.nn.functional.conv1d(xt, wt, bt, stride=key.stride, groups=key.G)[0].numpy().T
        if key.stride == 2:
            out[bi] = conv
        else:
            res = np.zeros((T, c_in))
            lo, hi = max(0, -res_shift), min(T, T - res_shift)
            res[lo:hi] = x[bi, lo + res_shift:hi + res_shift]
            out[bi] = res + ALPHA * (np.maximum(conv, 0.0) if relu else conv)
    return out


# ------------------------------------------------------------------------------------------------------------------
# the split form and the buffers
# ------------------------------------------------------------------------------------------------------------------
def encode_split(v):
    """[rows, C] (C % 32 == 0) -> uint16 [rows, C // 32, 64]: per 32-channel block 32 hi halves, then 32 lo halves;
    hi = fp16(v), lo = fp16((v - hi) * 2^11) (include/tal_asrd.h)."""
    v = np.asarray(v, dtype=np.float64)
    rows, C = v.shape
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float64)) * 2048.0).astype(np.float16)
    out = np.empty((rows, C // 32, 64), dtype=np.float16)
    out[:, :, :32] = hi.reshape(rows, C // 32, 32)
    out[:, :, 32:] = lo.reshape(rows, C // 32, 32)
    return out.view(np.uint16)


def decode_split(u16, rows, C):
    h = np.asarray(u16).view(np.float16).reshape(rows, C // 32, 2, 32).astype(np.float64)
    return (h[:, :, 0] + h[:, :, 1] / 2048.0).reshape(rows, C)


def banded_input(x, split, split_bytes=None):
    """[32 rows | x | 288 rows] as bytes, NaN in the bands -> (uint8 array, byte offset of the payload).  split: x in the split form
    (`split_bytes`: the payload as the library's tal_split_f16x3_fwd made it; default: encode_split)."""
    B, T, C = x.shape
    row = C * 4
    if split:
        pay = np.asarray(split_bytes, dtype=np.uint8) if split_bytes is not None else encode_split(x.reshape(B * T, C)).view(np.uint8).reshape(-1)
        buf = np.full((FRONT + B * T + BACK) * row, 0x7E, dtype=np.uint8)
    else:
        pay = np.ascontiguousarray(x, dtype=np.float32).view(np.uint8).reshape(-1)
        buf = np.empty((FRONT + B * T + BACK) * row, dtype=np.uint8)
        buf.view(np.uint32)[:] = 0x7FC00000
    assert pay.size == B * T * row
    buf[FRONT * row:FRONT * row + pay.size] = pay
    return buf, FRONT * row


def with_nan_band(payload, halves=False):
    """payload bytes | padding to 16 | AUX_BAND bytes of NaN (fp32 quiet NaNs, or NaN halves for fragment tables)."""
    pay = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
    n = (pay.size + 15) // 16 * 16
    buf = np.empty(n + AUX_BAND, dtype=np.uint8)
    if halves:
        buf[:] = 0x7E
    else:
        buf.view(np.uint32)[:] = 0x7FC00000
    buf[:pay.size] = pay
    return buf


def out_specs(case):
    """[(form, rows, C)] of the call's outputs."""
    key = case.key
    return [(form, key.B * out_len(key), key.G * key.cog) for form in ENTRIES[case.entry][2]]


def blank_output(rows, C):
    return np.full((FRONT + rows + BACK) * C * 4, FILL, dtype=np.uint8)


def filled_output(form, values):
    """The banded output buffer a perfect kernel leaves for `values` [rows, C]."""
    rows, C = values.shape
    buf = blank_output(rows, C)
    pay = values.astype(np.float32).view(np.uint8) if form == "f32" else encode_split(values).view(np.uint8)
    buf[FRONT * C * 4:(FRONT + rows) * C * 4] = pay.reshape(-1)
    return buf


def perfect_outputs(case, values=None):
    m = model(case.key) if values is None else values
    return [filled_output(form, m.reshape(rows, C)) for form, rows, C in out_specs(case)]


def check(case, bufs):
    """The three assertions on the raw bytes of the call's outputs (one uint8 array per output, bands included)."""
    key = case.key
    want = model(key)
    t_out = out_len(key)
    specs = out_specs(case)
    assert len(bufs) == len(specs), case.name
    for (form, rows, C), buf in zip(specs, bufs):
        buf = np.asarray(buf, dtype=np.uint8).reshape(-1)
        row = C * 4
        assert buf.size == (FRONT + rows + BACK) * row, "%s: buffer of %d bytes" % (case.name, buf.size)
        for what, band, first in (("in front of", buf[:FRONT * row], -FRONT), ("behind", buf[(FRONT + rows) * row:], rows)):
            bad = np.flatnonzero(band != FILL)
            assert bad.size == 0, "%s (%s output): %d bytes written %s the output, the first in row %d at byte %d" % (
                case.name, form, bad.size, what, first + bad[0] // row, bad[0] % row)
        pay = buf[FRONT * row:(FRONT + rows) * row]
        got = pay.view(np.float32).astype(np.float64).reshape(rows, C) if form == "f32" else decode_split(pay.view(np.uint16), rows, C)
        for what, bad in (("not finite", ~np.isfinite(got)), ("differs from the model", got != want.reshape(rows, C))):
            if bad.any():
                r, c = np.argwhere(bad)[0]
                raise AssertionError("%s (%s output): %d elements %s; the first at (b, t, channel) = (%d, %d, %d): got %r, the model has %r" % (
                    case.name, form, int(bad.sum()), what, r // t_out, r % t_out, c, got[r, c], want.reshape(rows, C)[r, c]))


# ------------------------------------------------------------------------------------------------------------------
# mutants: name -> function(case) -> list of output buffers, or None where the mutant does not apply to the case
# ------------------------------------------------------------------------------------------------------------------
def _model_mutant(applies, **knobs):
    def make(case):
        return perfect_outputs(case, wrong_model(case.key, **knobs)) if applies(case.key) else None
    return make


def _byte_mutant(edit):
    def make(case):
        bufs = perfect_outputs(case)
        return bufs if edit(case, bufs) is not False else None
    return make


def _poke(offset_rows):
    def edit(case, bufs):
        form, rows, C = out_specs(case)[-1]
        bufs[-1][(FRONT + rows + offset_rows if offset_rows >= 0 else FRONT + offset_rows) * C * 4 + 5] ^= 0x01
    return edit


def _leave_row(which):
    def edit(case, bufs):
        if which == "item1" and case.key.B < 2:
            return False
        for (form, rows, C), buf in zip(out_specs(case), bufs):
            r = rows - 1 if which == "last" else out_len(case.key)
            buf[(FRONT + r) * C * 4:(FRONT + r + 1) * C * 4] = FILL
    return edit


def _extra_row(case):
    """T_in = 2 T_out + 20: the odd last row taken as one more window start -- every item has T_out + 1 rows (the last one from a
    window that runs one row past the item), stored back to back."""
    key = case.key
    if key.stride != 2 or (key.T - key.k) % 2 == 0:
        return None
    longer = key._replace(T=key.T + 1)
    w, b = weights(key.stride, key.cig, key.cog, key.G, key.k)
    x = np.concatenate([x_of(key), np.zeros((key.B, 1, key.G * key.cig), dtype=np.float32)], axis=1)
    y = reference(x, w, b, 2, key.G)
    assert y.shape[1] == out_len(key) + 1 == out_len(longer)
    bufs = []
    for form, rows, C in out_specs(case):
        full = filled_output(form, y.reshape(-1, C))                       # rows + B payload rows
        buf = blank_output(rows, C)
        n = (FRONT + rows + key.B) * C * 4
        buf[:n] = full[:n]
        bufs.append(buf)
    return bufs


def _split_edit(fn):
    def make(case):
        if "split" not in ENTRIES[case.entry][2]:
            return None
        bufs = perfect_outputs(case)
        for (form, rows, C), buf in zip(out_specs(case), bufs):
            if form == "split":
                pay = buf[FRONT * C * 4:(FRONT + rows) * C * 4].view(np.uint16).reshape(rows, C // 32, 2, 32)
                fn(pay)
        return bufs
    return make


def _zero_lo(pay):
    pay[:, :, 1] = 0


def _swap_hi_lo(pay):
    pay[:, 1] = pay[:, 1, ::-1].copy()


def _swap_16_17(case):
    key = case.key
    if key.cog != 18:
        return None
    m = model(key).reshape(-1, key.G, 18).copy()
    m[:, :, [16, 17]] = m[:, :, [17, 16]]
    return perfect_outputs(case, m.reshape(model(key).shape))


_S1 = lambda key: key.stride == 1
_S2 = lambda key: key.stride == 2
_B2 = lambda key: key.B >= 2
MUTANTS = {
    "back_band_written": _byte_mutant(_poke(0)),
    "back_band_written_far": _byte_mutant(_poke(BACK - 1)),
    "front_band_written": _byte_mutant(_poke(-1)),
    "last_row_not_stored": _byte_mutant(_leave_row("last")),
    "first_row_of_item_1_not_stored": _byte_mutant(_leave_row("item1")),
    "taps_reversed": _model_mutant(lambda key: key.k > 1, flip=True),
    "padding_9": _model_mutant(_S1, shift=-1),
    "padding_11": _model_mutant(_S1, shift=1),
    "no_padding_between_items": _model_mutant(lambda key: _S1(key) and _B2(key), ends="neighbour"),
    "s2_windows_start_at_2t_plus_1": _model_mutant(_S2, s2_off=1),
    "s2_odd_last_row_is_a_window": _extra_row,
    "relu_missing": _model_mutant(_S1, relu=False),
    "residual_from_row_t_minus_1": _model_mutant(_S1, res_shift=-1),
    "residual_from_row_t_plus_1": _model_mutant(_S1, res_shift=1),
    "split_lo_zeroed": _split_edit(_zero_lo),
    "split_hi_lo_swapped_in_one_block": _split_edit(_swap_hi_lo),
    "channels_16_17_exchanged": _swap_16_17,
    "conv_over_the_poisoned_buffer": _model_mutant(_S1, ends="poison"),
}


# ------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------
T_S1 = (1, 2, 9, 10, 11, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)
TOUT_S2 = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 150)
SHORT, LONG = 1 << 20, 0        # gconv_short_below: 64-step tiles always / never
CASES = []


def _add(entry, key, opts=(), same=None):
    opts = tuple(sorted(dict(opts).items()))
    name = "%s-s%d-%dto%d-G%d-k%d-B%d-T%d" % ((entry,) + tuple(key)) + "".join("-%s%d" % (o.replace("gconv_", ""), v) for o, v in opts)
    CASES.append(Case(name, entry, key, opts, same))


def _valu(stride, cig, cog, G, B, T, opts=()):
    """The k = 21 VALU entry point and the any-k entry point at k = 21, which the project calls bit-identical."""
    key = Key(stride, cig, cog, G, 21, B, T)
    same = ("valu", key)
    _add("res" if stride == 1 else "s2", key, opts, same)
    if not opts:
        _add("res_k" if stride == 1 else "s2_k", key, (), same)


def _s2_lengths(touts, k=21):
    return [2 * to + k - 2 + odd for to in touts for odd in (0, 1)]


def _tile_forms(stride, cig, full):
    """(gconv_short_below, gconv_long_tt, gconv_grid_xyz) settings: 64-step tiles, the long tiles at their default length, the long
    tiles forced to 128 and 256 steps (read by the 10- and 14-channel stride-1 launches; elsewhere once, on the multi-tile cases:
    `full`), and the plain 3-D grid on `full` cases."""
    forms = [(SHORT, 0, 0), (LONG, 0, 0)]
    if (stride == 1 and cig in (10, 14)) or full:
        forms += [(LONG, 128, 0), (LONG, 256, 0)]
    if full:
        forms += [(SHORT, 0, 1), (LONG, 0, 1), (LONG, 128, 1), (LONG, 256, 1), (SHORT, 128, 0), (SHORT, 256, 1)]
    return forms


def _mfma(entry, key, full, extra=()):
    for below, long_tt, xyz in _tile_forms(key.stride, key.cig, full):
        opts = dict(extra, gconv_short_below=below, gconv_long_tt=long_tt, gconv_grid_xyz=xyz)
        _add(entry, key, opts, (entry, key, tuple(extra)))


def _mfma_entries(key, full, split_forms=True):
    C_in, C_out = channels(key)
    if key.stride == 1:
        _mfma("res_f16x3", key, full)
        if C_out % 32 == 0 and split_forms:
            _mfma("res_f16x3_ys", key, full)
            for no_shift in ((0, 1) if key.cig == 18 else (0,)):
                _mfma("res_split", key, full, (("gconv_no_shift18", no_shift),))
    else:
        _mfma("s2_f16x3", key, full)
        if C_out % 32 == 0 and split_forms:
            _mfma("s2_split_f32in", key, full)
            if C_in % 32 == 0:
                _mfma("s2_split", key, full)


def _build():
    # --- fp32 VALU kernels, k = 21 (and the any-k kernels at k = 21) -------------------------------------------------
    for cg in (10, 14, 18):
        for T in T_S1:
            for B in (1, 2):
                _valu(1, cg, cg, 16, B, T)
        for G in (80, 40, 64):
            _valu(1, cg, cg, G, 1, 300)
            _valu(1, cg, cg, G, 2, 17)
    for T in (1, 10, 11, 64, 257):
        _valu(1, 4, 4, 8, 2, T)                                  # gconv_generic_kernel
    for cig, cog in ((1, 10), (10, 14), (14, 18)):
        for T in _s2_lengths(TOUT_S2):
            for B in (1, 2):
                _valu(2, cig, cog, 16, B, T)                     # (1 -> 10, G = 16: launch_spec<1, 10, 2, 16, 128>)
        for G in (80, 40, 64):                                   # (1 -> 10: G = 80 / 40 the channel-major kernel, 32-step tiles)
            _valu(2, cig, cog, G, 1, 320)
            _valu(2, cig, cog, G, 2, 53)
    for T in _s2_lengths((1, 17, 64, 129)):
        _valu(2, 2, 3, 8, 2, T)                                  # gconv_generic_kernel
        _valu(2, 1, 10, 8, 2, T)                                 # 1 -> 10 on the generic kernel (G % 16 != 0)
        _valu(2, 1, 10, 20, 2, T, (("gconv_c1_generic", 1),))    # ... by option (G % 16 != 0: generic)
        _valu(2, 1, 10, 80, 2, T, (("gconv_c1_generic", 1),))    # ... by option (G % 16 == 0: the slab kernel)
    for T in (21, 85, 600):
        _valu(2, 1, 10, 80, 64, T)                               # channel-major kernel, 256-step tiles: cdiv(T_out, 256) * 4 * 64 >= 256
    _valu(2, 1, 10, 80, 1, 600)                                  # ... 32-step tiles
    # --- any-k kernels ------------------------------------------------------------------------------------------------
    for k in (1, 3, 15, 31, 63):
        ts = sorted({1, max(k // 2, 1), k // 2 + 1, k, 64, 255, 256, 257, 300})
        for cg, G in ((10, 16), (14, 16), (18, 16), (10, 3), (4, 8)):       # vector arm x 3; C % 4 != 0 with an odd group count; any width
            for T in ts:
                _add("res_k", Key(1, cg, cg, G, k, 2, T))
            _add("res_k", Key(1, cg, cg, G, k, 1, 257))
    for k in (1, 3, 8, 15, 31, 63):
        for cig, cog, G in ((1, 10, 20), (10, 14, 16), (14, 18, 16), (10, 14, 3), (2, 3, 8)):
            for T in _s2_lengths((1, 17, 64, 65, 129), k):
                _add("s2_k", Key(2, cig, cog, G, k, 2, T))
            _add("s2_k", Key(2, cig, cog, G, k, 1, 2 * 129 + k - 1))
    for k in (8, 21, 63):
        _add("s2_k", Key(2, 1, 10, 80, k, 64, 2 * 33 + k - 1))   # gconv_k_c1_kernel<128>: cdiv(T_out, 128) * 4 * 64 >= 256
    # --- matrix-core kernels ------------------------------------------------------------------------------------------
    for cg in (10, 14, 18):
        for T in T_S1:
            for B in (1, 2):
                _mfma_entries(Key(1, cg, cg, 16, 21, B, T), full=(T in (17, 257, 300)))
        for G in (80, 40, 64):
            _mfma_entries(Key(1, cg, cg, G, 21, 1, 300), full=False)
            _mfma_entries(Key(1, cg, cg, G, 21, 2, 17), full=False)
    for T, B in ((300, 1), (17, 2), (257, 2)):
        _mfma_entries(Key(1, 18, 18, 12, 21, B, T), full=True)   # 6 group blocks: the grid is no multiple of 8
    for cig, cog in ((10, 14), (14, 18)):
        for T in _s2_lengths(TOUT_S2):
            for B in (1, 2):
                _mfma_entries(Key(2, cig, cog, 16, 21, B, T), full=(T in (53, 54, 277, 278, 319, 320)))
        for G in (80, 40, 64):
            _mfma_entries(Key(2, cig, cog, G, 21, 1, 320), full=False)
            _mfma_entries(Key(2, cig, cog, G, 21, 2, 53), full=False)


_build()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
