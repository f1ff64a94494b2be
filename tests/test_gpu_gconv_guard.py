"""Every grouped-conv entry point of the C ABI inside guard bands, against the exact model of tests/_gconv_ref.py.  pytest -m gpu.

The test calls lib.tal_gconv_* itself.  x sits between NaN bands ([32 rows | x | 288 rows]), bias / packed weights / fragments are
followed by NaN bands, every output lies in [32 rows | payload | 288 rows] of bytes 0x5A.  R.check then wants the output bands byte-
identical to the fill (no store in front of row 0 or past the last row), every payload element finite (nothing outside the input was
read: NaN * 0 is NaN) and the payload EQUAL to the float64 model -- the data are small integers, every sum is exact in any order
(tests/test_gconv_ref_cpu.py asserts the premises and that each plausible wrong kernel is rejected).  There is no tolerance in this
file except LOGIT_TOL of the driver-level test.  Forms of one problem that the project calls bit-identical (64-step, 128-step and
256-step tiles, the XCD-ordered and the plain grid, the any-k kernel at k = 21) are compared byte for byte as they come by.

  kernel / arm (csrc/gconv.hip, csrc/gconv_general.hip)          cases (R.CASES names: entry-s<stride>-<cig>to<cog>-G..-k..-B..-T..)
  gconv_kernel<10|14|18, stride 1, 2 groups x 256>                res-s1-*-G16 (all of T_S1 x B 1, 2), -G80 / -G40 / -G64
  gconv_kernel<10->14 (4 x 128), 14->18 (2 x 128), stride 2>      s2-s2-10to14-*, s2-s2-14to18-* (T_in = 2 T_out + 19 and + 20)
  gconv_kernel<1->10, 16 groups x 128>                            s2-s2-1to10-G16-*, -G64-*, -G80-*-c1_generic1
  gconv_generic_kernel (both forms)                               res-s1-4to4-G8-*, s2-s2-2to3-G8-*, s2-s2-1to10-G8-*, -G20-*-c1_generic1
  gconv_s2_c1_kernel<32-step>                                     s2-s2-1to10-G80-*-B1-T320 / -B2-T53 / -B1-T600, -G40-*
  gconv_s2_c1_kernel<256-step> (clamped loads, almost empty tile) s2-s2-1to10-G80-k21-B64-T21 / -T85 / -T600
  gconv_s2_c1_kernel<.., split output>, fused first conv          test_encoder_call_inside_guard_bands (reachable through tal_tds_fwd only)
  gconv_k_kernel (vector arm), every width                        res_k-*-G16-k{1,3,15,21,31,63}-*, s2_k-*-G16-k{1,3,8,15,21,31,63}-*
  gconv_k_any_kernel: C % 4 != 0 with an odd group count; width   res_k-s1-10to10-G3-*, s2_k-s2-10to14-G3-*; res_k-s1-4to4-G8-*, s2_k-s2-2to3-G8-*
  gconv_k_c1_kernel<32>, <128>                                    s2_k-s2-1to10-G20-*; s2_k-s2-1to10-G80-k{8,21,63}-B64-*
  gconv_mfma_kernel<10|14|18, 64 / 128 / 256 steps, fp32 out>     res_f16x3-*-short_below{1048576,0}-long_tt{0,128,256}
  ... fp32 + split out                                            res_f16x3_ys-*
  ... split in, split out; gconv18_shift_kernel<64>, <256>        res_split-*-no_shift18{1,0}-*
  gconv_mfma_kernel<10->14, 14->18, 64 / 128 steps>               s2_f16x3-*, s2_split_f32in-*, s2_split-* (x_is_split 0 / 1)
  XCD-ordered grid / plain grid; n_gb = 4, 8, 10, 16, 20, 32, 40  *-grid_xyz{0,1}; -G16 / -G40 / -G64 / -G80
  a grid that is no multiple of 8                                 res_f16x3-s1-18to18-G12-* (6 group blocks)
  halo (10 rows), 16-step blocks, 64 / 128 / 256-step tiles       T_S1 = 1 .. 300 on every stride-1 entry; T_out = 1 .. 150 on every stride-2 entry
  odd last input row of a stride-2 conv                           T_in = 2 T_out + 20
  an overrun of item 0 into item 1                                every B2 case (the model is compared element by element)
"""
import ctypes as C
import hashlib
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import _gconv_ref as R
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

_SEEN = {}          # Case.same -> (case name, digests of the raw outputs) of the first form that ran


def dev():
    return torch.device("cuda:0")


def _up(a):
    return torch.from_numpy(np.array(a)).to(dev())      # (a copy: the table's arrays are read-only)


def _band_intact(buf, used, fill, what):
    assert bool((buf[used:] == fill).all()), "%s: bytes behind the payload were written" % what


@lru_cache(maxsize=None)
def _bias_dev(stride, cig, cog, G, k):
    _, b = R.weights(stride, cig, cog, G, k)
    return _up(R.with_nan_band(b.astype(np.float32)))


@lru_cache(maxsize=None)
def _packed_dev(stride, cig, cog, G, k):
    """The packed fp32 weights behind a NaN band; tal_pack_gconv_weight, run into such a buffer, gives the same bytes."""
    from tal_asrd_amd import _native as N
    w, _ = R.weights(stride, cig, cog, G, k)
    want = _up(R.with_nan_band(R.pack_weight(w, G)))
    got = _up(R.with_nan_band(np.zeros(w.size, dtype=np.float32)))
    src = _up(w.astype(np.float32))
    N.check(N.lib().tal_pack_gconv_weight(N.ptr(src), N.ptr(got), G * cog, cig, k, G, N.stream_handle()), "tal_pack_gconv_weight")
    torch.cuda.synchronize()
    assert torch.equal(got, want), "tal_pack_gconv_weight: not the documented layout, or it wrote behind its output"
    return want


@lru_cache(maxsize=None)
def _frag_dev(stride, cig, cog, G):
    """The fp16x3 MFMA fragments of the case's weights, packed by the library into [fragments | NaN halves]."""
    from tal_asrd_amd import _native as N
    lib = N.lib()
    w, _ = R.weights(stride, cig, cog, G, 21)
    nbytes = lib.tal_gconv_f16x3_weight_bytes(G * cig, G * cog, G, stride)
    assert nbytes > 0 and nbytes % 16 == 0, (stride, cig, cog, G, nbytes)
    buf = torch.full((nbytes + R.AUX_BAND,), 0x7E, dtype=torch.uint8, device=dev())
    src = _up(w.astype(np.float32))
    N.check(lib.tal_pack_gconv_f16x3_weight(N.ptr(src), N.ptr(buf), G * cig, G * cog, G, stride, N.stream_handle()), "tal_pack_gconv_f16x3_weight")
    torch.cuda.synchronize()
    _band_intact(buf, nbytes, 0x7E, "tal_pack_gconv_f16x3_weight")
    assert bool(torch.isfinite(buf[:nbytes].view(torch.float16)).all())
    return buf


@lru_cache(maxsize=6)
def _x_dev(key, split):
    """x between its NaN bands on the device -> (buffer, the payload as a view of it).  split: tal_split_f16x3_fwd of the exact data."""
    from tal_asrd_amd import ops
    x = R.x_of(key)
    if split:
        xs = ops.split_f16x3(_up(x.reshape(key.B * key.T, -1)))
        torch.cuda.synchronize()
        host, off = R.banded_input(x, True, xs.cpu().numpy())
    else:
        host, off = R.banded_input(x, False)
    buf = _up(host)
    return buf, buf[off:off + x.size * 4]


def _call(lib, N, entry, key, x, w, bias, alpha, outs):
    """One call of the entry point on the problem `key`; every argument is a device pointer to a payload."""
    fn = getattr(lib, R.ENTRIES[entry][0])
    C_in, C_out = R.channels(key)
    st = N.stream_handle()
    x, w, bias = N.ptr(x), N.ptr(w), N.ptr(bias)
    o = [N.ptr(t) for t in outs]
    if entry == "res":
        return fn(x, w, bias, alpha, key.B, key.T, C_in, key.G, o[0], st)
    if entry == "s2":
        return fn(x, w, bias, key.B, key.T, C_in, C_out, key.G, o[0], st)
    if entry == "res_k":
        return fn(x, w, bias, alpha, key.B, key.T, C_in, key.G, key.k, o[0], st)
    if entry == "s2_k":
        return fn(x, w, bias, key.B, key.T, C_in, C_out, key.G, key.k, o[0], st)
    if entry == "res_f16x3":
        return fn(x, w, bias, alpha, key.B, key.T, C_in, key.G, o[0], None, st)
    if entry == "res_f16x3_ys":
        return fn(x, w, bias, alpha, key.B, key.T, C_in, key.G, o[0], o[1], st)
    if entry == "s2_f16x3":
        return fn(x, w, bias, key.B, key.T, C_in, C_out, key.G, o[0], st)
    if entry == "res_split":
        return fn(x, w, bias, alpha, key.B, key.T, C_in, key.G, o[0], st)
    assert entry in ("s2_split", "s2_split_f32in")
    return fn(x, 1 if entry == "s2_split" else 0, w, bias, key.B, key.T, C_in, C_out, key.G, o[0], st)


def banded_call(entry, key, x, w, bias, alpha=R.ALPHA, opts=(), what=""):
    """The entry point on payload x (a device tensor inside its own bands, or not) with every output inside [32 rows | payload |
    288 rows] of bytes 0x5A, under the options `opts` -> the raw output buffers on the device, bands included."""
    from tal_asrd_amd import _native as N
    lib = N.lib()
    t_out = R.out_len(key)
    C_out = key.G * key.cog
    rows, row = key.B * t_out, C_out * 4
    bufs = [torch.full(((R.FRONT + rows + R.BACK) * row,), R.FILL, dtype=torch.uint8, device=dev()) for _ in R.ENTRIES[entry][2]]
    outs = [b[R.FRONT * row:(R.FRONT + rows) * row] for b in bufs]
    try:
        for name, value in opts:
            N.set_option(name, value)
        rc = _call(lib, N, entry, key, x, w, bias, alpha, outs)
    finally:
        for name, value in R.OPTION_DEFAULTS.items():
            N.set_option(name, value)
    N.check(rc, what or entry)
    torch.cuda.synchronize()
    return bufs


def run_case(case):
    """The case's call on its banded inputs -> the raw bytes of its outputs (numpy, one array per output)."""
    key = case.key
    wkey = (key.stride, key.cig, key.cog, key.G, key.k)
    w = _frag_dev(key.stride, key.cig, key.cog, key.G) if case.entry in R.MFMA_ENTRIES else _packed_dev(*wkey)
    _, x = _x_dev(key, R.ENTRIES[case.entry][1])
    return [b.cpu().numpy() for b in banded_call(case.entry, key, x, w, _bias_dev(*wkey), R.ALPHA, case.opts, case.name)]


def guarded_f16x3(x, w_frag, bias, G, c_out=None, alpha=None, want_split=False):
    """ops.gconv_res_f16x3 (alpha given) / ops.gconv_s2_f16x3 (c_out given) for the tolerance tests on random data
    (tests/test_gpu_parity.py, tests/test_gpu_stress.py), run through the banded buffers: x [B, T, C] fp32 between NaN bands, the
    bias behind one, every output between bands of 0x5A that must come back untouched -> y [B, T_out, C_out] (and its split form)."""
    B, T, C_in = x.shape
    stride = 1 if alpha is not None else 2
    c_out = C_in if stride == 1 else c_out
    key = R.Key(stride, C_in // G, c_out // G, G, 21, B, T)
    entry = ("res_f16x3_ys" if want_split else "res_f16x3") if stride == 1 else "s2_f16x3"
    host, off = R.banded_input(x.detach().cpu().numpy(), False)
    xbuf = _up(host)
    bbuf = _up(R.with_nan_band(bias.detach().cpu().numpy().astype(np.float32)))
    bufs = banded_call(entry, key, xbuf[off:off + x.numel() * 4], w_frag, bbuf, 0.0 if alpha is None else float(alpha))
    rows, row = B * R.out_len(key), c_out * 4
    for buf in bufs:
        assert bool((buf[:R.FRONT * row] == R.FILL).all()), "rows in front of the output were written"
        assert bool((buf[(R.FRONT + rows) * row:] == R.FILL).all()), "rows behind the output were written"
    pay = [buf[R.FRONT * row:(R.FRONT + rows) * row].clone() for buf in bufs]
    y = pay[0].view(torch.float32).reshape(B, R.out_len(key), c_out)
    return (y, pay[1]) if want_split else y


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_entry_point_inside_guard_bands(name):
    case = R.CASE_BY_NAME[name]
    got = run_case(case)
    R.check(case, got)
    if case.same is not None:
        digests = [hashlib.sha1(b.tobytes()).digest() for b in got]
        first = _SEEN.setdefault(case.same, (case.name, digests))
        assert first[1] == digests, "%s and %s are called bit-identical and differ" % (first[0], case.name)


def test_inputs_are_left_as_they_were():
    """No entry point writes to x, bias or weights: after the whole table has run (or none of it), the cached device buffers still
    hold what was uploaded."""
    case = R.CASE_BY_NAME["res_split-s1-18to18-G16-k21-B2-T300-grid_xyz0-long_tt0-no_shift180-short_below0"]
    key = case.key
    buf, _ = _x_dev(key, True)
    before = buf.clone()
    R.check(case, run_case(case))
    assert torch.equal(buf, before)
    wkey = (key.stride, key.cig, key.cog, key.G, key.k)
    _, b = R.weights(*wkey)
    assert torch.equal(_bias_dev(*wkey), _up(R.with_nan_band(b.astype(np.float32))))
    frag = _frag_dev(key.stride, key.cig, key.cog, key.G)
    _band_intact(frag, frag.numel() - R.AUX_BAND, 0x7E, "fragments")


# ------------------------------------------------------------------------------------------------------------------
# the encoder driver: the only way to the split-writing 1 -> 10 kernel and to the fused first conv
# ------------------------------------------------------------------------------------------------------------------
SETTINGS = ["default", "tds_fp32_activations", "exact_flag", "gconv_general", "gconv_c1_fuse"]
WS_BAND = 1 << 20


@pytest.fixture(scope="module")
def encoder(sd_weights):
    from tal_asrd_amd import SDModel, synth
    from tests.test_gpu_parity import _load
    model = _load(SDModel(), sd_weights)
    enc = model.encoder
    assert list(enc.sizes) == [80, 800, 1120, 1440]
    state = {"model": model, "desc": enc._descriptor(0, len(enc.sizes) - 1), "mel": {}, "exact": {}}

    def mel(T):
        if T not in state["mel"]:
            audio = torch.from_numpy(synth.synth_audio_batch(1, (T - 1) * 160, 4321)).to(dev())
            with torch.no_grad():
                m = model.extract_features(audio)
            assert tuple(m.shape) == (1, T, 80)
            state["mel"][T] = m.contiguous()
        return state["mel"][T]
    state["mel_of"] = mel
    return state


def _shortest_all_split_length(desc):
    """The shortest T at which the last stage runs all-split (tds_blocks_split_ok: more than 128 rows into its blocks)."""
    from tal_asrd_amd import _native as N
    lib = N.lib()
    asked = N.TdsDesc.from_buffer_copy(desc)
    asked.flags |= N.TAL_TDS_OUT_SPLIT
    lo, hi = 1, 4096
    assert lib.tal_tds_out_split(C.byref(asked), 1, hi) == 1
    while hi - lo > 1:                       # (monotone in T: the row counts only grow)
        mid = (lo + hi) // 2
        if lib.tal_tds_out_split(C.byref(asked), 1, mid) == 1:
            hi = mid
        else:
            lo = mid
    assert lib.tal_tds_out_split(C.byref(asked), 1, hi - 1) == 0
    return hi


def _encoder_call(desc, mel, flags):
    """tal_tds_fwd with x between NaN bands, y between 0x5A bands and a workspace of exactly tal_tds_workspace_bytes inside a larger
    0x5A-filled allocation -> (y payload as float64 [T', 1440], range word, form word)."""
    from tal_asrd_amd import _native as N
    lib = N.lib()
    d = N.TdsDesc.from_buffer_copy(desc)
    d.flags |= flags
    B, T, _ = mel.shape
    host, off = R.banded_input(mel.cpu().numpy(), False)
    xbuf = _up(host)
    x = xbuf[off:off + mel.numel() * 4]
    t_out = lib.tal_tds_out_len(C.byref(d), T)
    row = 1440 * 4
    ybuf = torch.full(((R.FRONT + B * t_out + R.BACK) * row,), R.FILL, dtype=torch.uint8, device=dev())
    y = ybuf[R.FRONT * row:(R.FRONT + B * t_out) * row]
    nws = lib.tal_tds_workspace_bytes(C.byref(d), B, T)
    wsbuf = torch.full((WS_BAND + nws + WS_BAND,), R.FILL, dtype=torch.uint8, device=dev())
    ws = wsbuf[WS_BAND:WS_BAND + nws]
    N.check(lib.tal_tds_fwd(C.byref(d), N.ptr(x), B, T, N.ptr(y), N.ptr(ws), nws, N.stream_handle()), "tal_tds_fwd")
    torch.cuda.synchronize()
    assert torch.equal(xbuf, _up(host)), "x or its bands were written"
    assert bool((ybuf[:R.FRONT * row] == R.FILL).all()) and bool((ybuf[(R.FRONT + B * t_out) * row:] == R.FILL).all()), "bytes around y were written"
    assert bool((wsbuf[:WS_BAND] == R.FILL).all()) and bool((wsbuf[WS_BAND + nws:] == R.FILL).all()), "bytes around the workspace were written"
    so = lib.tal_tds_status_offset(C.byref(d), B, T)
    flag, form = ws[so:so + 8].view(torch.int32).tolist()
    pay = y.cpu().numpy()
    got = R.decode_split(pay.view(np.uint16), B * t_out, 1440) if form else pay.view(np.float32).astype(np.float64).reshape(B * t_out, 1440)
    return got, flag, form, lib.tal_tds_out_split(C.byref(d), B, T)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("length", ["shortest_all_split", "T1200"])
def test_encoder_call_inside_guard_bands(encoder, length, setting):
    """tal_tds_fwd on the full-size synthetic encoder (80 / 800 / 1120 / 1440, depths 2 / 3 / 6) and a log-mel input: nothing is
    written around x, y or the workspace, the range word stays 0, the output is finite and within LOGIT_TOL of the call on the exact
    fp32 kernels.  The shortest all-split length runs with TAL_TDS_OUT_SPLIT (the default and the fused first conv then write the
    split form), T = 1200 without."""
    from tal_asrd_amd import _native as N
    from tests.test_gpu_parity import LOGIT_TOL
    desc = encoder["desc"]
    T = _shortest_all_split_length(desc) if length == "shortest_all_split" else 1200
    out_flag = N.TAL_TDS_OUT_SPLIT if length == "shortest_all_split" else 0
    mel = encoder["mel_of"](T)
    if T not in encoder["exact"]:
        want, flag, form, _ = _encoder_call(desc, mel, N.TAL_TDS_EXACT_F32)
        assert flag == 0 and form == 0 and np.isfinite(want).all()
        encoder["exact"][T] = want
    want = encoder["exact"][T]
    opts = {setting: 1} if setting in ("tds_fp32_activations", "gconv_general", "gconv_c1_fuse") else {}
    flags = out_flag | (N.TAL_TDS_EXACT_F32 if setting == "exact_flag" else 0)
    try:
        for k, v in opts.items():
            N.set_option(k, v)
        got, flag, form, predicted = _encoder_call(desc, mel, flags)
    finally:
        for k in opts:
            N.set_option(k, 0)
    assert flag == 0, "the range word was raised"
    assert form == predicted == (1 if out_flag and setting in ("default", "gconv_c1_fuse") else 0), (length, setting, form, predicted)
    assert got.shape == want.shape and np.isfinite(got).all()
    err = float(np.abs(got - want).max())
    print("encoder %s %s: T=%d form=%d max |y - exact| = %.3e" % (length, setting, T, form, err))
    assert err < LOGIT_TOL, (length, setting, err)
    if setting == "exact_flag":
        assert np.array_equal(got, want)
