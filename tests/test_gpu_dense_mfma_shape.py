"""The fp16x3 dense layers on 16x16x32 MFMAs (csrc/gemm_w64.hip, the F16X3 branch of gemm_glds_kernel in csrc/gemm_f32.hip, the
16x16 staging write of csrc/gemm_common.h), GPU.

1. An exact integer model through every dispatch form.  The operands are built on the host directly in the split format with
   small integer halves, so that every partial sum is exact in fp32 whatever the summation order; the expected output is the
   integer model BIT FOR BIT.  A wrong lane -> row / column / k-group mapping, a dropped or doubled K block or a wrong
   accumulator cannot hide in a tolerance.
2. Random data against float64 with the project's dense-layer bound, bitwise repeatable.

Which form ran.  The C ABI does not say which kernel a call launched.  What a test can observe: the number of dense-layer
profiling scopes and their work (one scope with the whole 2 M N K: no row split into a second launch), and -- for the K-sliced
forms -- the split-K scratch, which the slices fill with whole tiles: the number of floats written is
tail tiles x slices x tile rows x 160, which tells the 256-row kernel from the 128-row kernel.  For the whole-tile forms
(256 x 160, 128 x 160, 128 x 96) the kernel is the dispatcher's choice at this tile count (launch_gemm, csrc/gemm_f32.hip);
each case asserts the inequalities that decide it, with the CU count of the device, and that the scratch stayed untouched.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

PROF_GEMM = 0


def dev():
    return torch.device("cuda:0")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _cdiv(a, b):
    return -(-a // b)


def _pack(hi, lo):
    """the fp16x3 operand format (include/tal_asrd.h, _np_split in tests/test_gpu_parity.py): per row and 32-wide K block,
    32 hi halves then 32 lo halves"""
    rows, K = hi.shape
    out = np.empty((rows, K // 32, 64), dtype=np.float16)
    out[:, :, :32] = hi.reshape(rows, K // 32, 32)
    out[:, :, 32:] = lo.reshape(rows, K // 32, 32)
    return out


def _host_split(y):
    """host split of exact fp32 values inside the fp16 range: hi = fp16(y), lo = fp16((y - hi) * 2^11)"""
    hi = y.astype(np.float16)
    lo = ((y - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return _pack(hi, lo)


def _int_operand(rng, rows, K):
    hi = rng.integers(-2, 3, size=(rows, K)).astype(np.float32)
    lo = rng.integers(-8, 9, size=(rows, K)).astype(np.float32)
    return hi, lo


def _exact_problem(M, N, K):
    """operands with integer halves and the exact results of both layers.  Model: y = sum hi.hi' + b + 2^-11 sum (hi.lo' + lo.hi')
    (lo.lo' is dropped by the kernels by design).  Every term is an integer: the float64 products below are an int64 model,
    exact in any order; 4 K + 4 < 4096 keeps every fp32 partial sum of the kernel exact too."""
    assert 4 * K + 4 < 4096
    rng = np.random.default_rng(1000 * N + K)
    xh, xl = _int_operand(rng, M, K)
    wh, wl = _int_operand(rng, N, K)
    b = rng.integers(-4, 5, size=N).astype(np.float32)
    rh, rl = _int_operand(rng, M, N)          # the split residual of the mode-2 layer
    d = dev()
    t = lambda a: torch.from_numpy(a).to(d).double()
    hh = t(xh) @ t(wh).t()
    xx = t(xh) @ t(wl).t() + t(xl) @ t(wh).t()
    pre = hh + t(b) + xx / 2048.0
    assert float(pre.abs().max()) < 4 * K + 8
    y1 = pre.clamp_min(0.0)
    y2 = (t(rh) + t(rl) / 2048.0) + 0.5 * pre
    exp = {}
    for mode, y in ((1, y1), (2, y2)):
        y32 = y.float()
        assert torch.equal(y32.double(), y)                      # the model's values ARE fp32 values
        exp[mode] = y32.cpu().numpy()
    u8 = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1)).to(d)
    return dict(xs=u8(_pack(xh, xl)), ws=u8(_pack(wh, wl)), b=torch.from_numpy(b).to(d), rs=u8(_pack(rh, rl)), exp=exp)


_PROBLEMS = {}


def _problem(M, N, K):
    key = (M, N, K)
    if key not in _PROBLEMS:
        _PROBLEMS.clear()                    # (one at a time: the large ones are 100 MB on the device)
        _PROBLEMS[key] = _exact_problem(M, N, K)
    return _PROBLEMS[key]


GUARD = 5


def _launch(p, M, N, K, mode, out_split, guarded, scratch):
    """one dense layer; returns (output rows, floats of the split-K scratch that were written, profiling scopes, their work)"""
    from tal_asrd_amd import _native as N_
    lib = N_.lib()
    d = dev()
    if out_split:
        ybuf = torch.full(((M + GUARD) * N * 4,), 0x5A, dtype=torch.uint8, device=d)
    else:
        ybuf = torch.full((M + GUARD, N), 4321.0, device=d)
    scratch.fill_(0xFF)                      # NaN as fp32; a K slice writes whole tiles of finite partial sums
    flag = torch.zeros(16, dtype=torch.int32, device=d)
    res = p["rs"] if mode == 2 else None
    lib.tal_prof_reset()
    lib.tal_prof_enable(1)
    try:
        if guarded:
            N_.check(lib.tal_linear_f16x3_guarded_fwd(N_.ptr(p["xs"]), N_.ptr(p["ws"]), N_.ptr(p["b"]), N_.ptr(res) if res is not None else None,
                                                      1 if mode == 2 else 0, 0.5, mode, M, N, K, N_.ptr(ybuf), out_split, N_.ptr(flag),
                                                      N_.ptr(scratch), scratch.numel(), N_.stream_handle()), "tal_linear_f16x3_guarded_fwd")
        else:
            N_.check(lib.tal_linear_f16x3_fwd(N_.ptr(p["xs"]), N_.ptr(p["ws"]), N_.ptr(p["b"]), None, 0.5, mode, M, N, K, N_.ptr(ybuf), out_split,
                                              N_.ptr(scratch), scratch.numel(), N_.stream_handle()), "tal_linear_f16x3_fwd")
        torch.cuda.synchronize()
    finally:
        lib.tal_prof_enable(0)
    ms, n, work = C.c_double(), C.c_int64(), C.c_double()
    N_.check(lib.tal_prof_collect(PROF_GEMM, C.byref(ms), C.byref(n), C.byref(work)), "tal_prof_collect")
    assert int(flag.abs().sum()) == 0, "status word"
    if out_split:
        assert bool((ybuf[M * N * 4:] == 0x5A).all()), "wrote behind the output"
        y = ybuf[:M * N * 4]
    else:
        assert bool((ybuf[M:] == 4321.0).all()), "wrote behind the output"
        y = ybuf[:M]
    written = int((~torch.isnan(scratch.view(torch.float32))).sum())
    return y, written, int(n.value), float(work.value)


# (mode, split output, guarded call): relu -> fp32 (shared epilogue), split-form residual -> fp32 (shared epilogue, guarded),
# relu -> split form and split residual -> split form under the range guard (the static-addressing epilogue)
RUNS = [(1, 0, False), (2, 0, True), (1, 1, True), (2, 1, True)]


def _check_exact(M, N, K, options, expect_written, runs=RUNS):
    from tal_asrd_amd import _native as N_
    lib = N_.lib()
    p = _problem(M, N, K)
    nws = max(int(lib.tal_linear_workspace_bytes(M, N, K)), 16)
    scratch = torch.empty(nws, dtype=torch.uint8, device=dev())
    try:
        for name, value in options.items():
            N_.set_option(name, value)
        for mode, out_split, guarded in runs:
            what = (M, N, K, mode, out_split, guarded)
            y, written, scopes, work = _launch(p, M, N, K, mode, out_split, guarded, scratch)
            assert scopes == 1 and work == 2.0 * M * N * K, ("one dense launch scope with the whole work", what, scopes, work)
            assert written == expect_written(mode, out_split, guarded), ("split-K scratch floats written", what, written)
            if out_split:
                got = y.cpu().numpy().view(np.uint16)
                want = _host_split(p["exp"][mode]).view(np.uint16).reshape(-1)
                assert np.array_equal(got, want), what
            else:
                assert torch.equal(y.cpu(), torch.from_numpy(p["exp"][mode])), what
    finally:
        for name in options:
            N_.set_option(name, {"gemm_s64_below": 2}.get(name, 0))


def _not_short_input(M, N, cus):
    """launch_gemm's first arm: the 64 x 80 tiles take a launch of up to two workgroups per CU (option gemm_s64_below = 2)"""
    return _cdiv(M, 64) * (N // 80) > 2 * cus


# K = 32 .. 160: a prologue whose second tile is past the end, and every remainder of the K loop (unrolled by six: three operand
# buffers x two A fragment sets) short of one full pass; 192: exactly one pass, no remainder; 224: a pass and a remainder
@pytest.mark.parametrize("K", [32, 64, 96, 128, 160, 192, 224])
def test_exact_w64_whole_tiles(K):
    """256 x 160 tiles of gemm_w64_kernel, whole tiles only: one round and one more tile with 3 rows.  Form: CUs + 1 tiles of
    256 rows are at least one round (one workgroup per CU); the 3 remaining rows are too few for a launch of their own
    (<= 128), and K / 32 < 8 leaves no K slices (a slice has at least 4 K steps)."""
    cus = _cus()
    M, N = 256 * cus + 3, 160
    assert _not_short_input(M, N, cus) and _cdiv(M, 256) * _cdiv(N, 160) >= cus and M - 256 * cus <= 128 and K // 32 < 8
    _check_exact(M, N, K, {}, lambda *run: 0)


def test_exact_w64_rounds_and_k_sliced_tail():
    """one round of gemm_w64_kernel and 20 tail tiles cut into two K slices (nk = 8) behind it, added by the fix-up launch.
    Form: 5000 remaining rows are more than the 4096 that would go off as a launch of their own; the scratch holds
    20 tiles x 2 slices x 256 rows x 160 floats afterwards -- 128-row tiles would leave half as much per tile."""
    cus = _cus()
    M, N, K = 256 * cus + 5000, 160, 256
    assert _not_short_input(M, N, cus) and M - 256 * cus > 4096
    tail = _cdiv(M, 256) - cus
    _check_exact(M, N, K, {}, lambda *run: tail * 2 * 256 * 160)


@pytest.mark.parametrize("K", [96, 256])
def test_exact_glds_128x160_whole_tiles(K):
    """128 x 160 tiles of gemm_glds_kernel, option gemm_no_w64 left at 0: 8000 x 800 is 160 tiles of 256 rows, fewer than one
    round of the 256-row kernel, so the dispatcher goes on to the 128-row kernel: 315 tiles, more than a quarter of its round
    (two workgroups per CU) and less than one, which launch_gemm does not cut along K at any K -- K = 256 is a whole-tile case
    as well (both operand buffers four times); the K-sliced form is test_exact_glds_128x160_k_sliced."""
    cus = _cus()
    M, N = 8000, 800
    nb = _cdiv(M, 128) * (N // 160)
    assert _not_short_input(M, N, cus) and _cdiv(M, 256) * (N // 160) < cus and 4 * nb > 2 * cus and nb < 2 * cus and N % 96 != 0
    _check_exact(M, N, K, {}, lambda *run: 0)


def test_exact_glds_128x160_k_sliced():
    """gemm_glds_kernel's K-sliced launch with the raw-accumulator hand-over to gemm_splitk_fixup_kernel, K = 256.  The
    dispatcher cuts a launch of the 128-row kernel along K only if it has whole rounds in front of its tail (then the 256-row
    kernel has taken it) or is under a quarter of a round and its scratch traffic is small against a round: 700 x 800 is
    30 tiles, two slices each.  So few rows are a short input (64 x 80 tiles): option gemm_s64_below = 0 switches that arm
    off, as tests/test_gpu_parity.py does for the same purpose.  The scratch holds 30 x 2 x 128 x 160 floats afterwards."""
    cus = _cus()
    M, N, K = 700, 800, 256
    nb = _cdiv(M, 128) * (N // 160)
    assert 4 * nb <= 2 * cus and _cdiv(M, 256) * (N // 160) < cus
    _check_exact(M, N, K, {"gemm_s64_below": 0}, lambda *run: nb * 2 * 128 * 160)


def test_exact_glds_128x96_tiles():
    """128 x 96 tiles (gemm_glds_kernel<., 3, ...>): the row and column count of the `glds96` entry of tests/test_gpu_fp16x3_range.py
    (1819 x 1440: the fewest rows that are no short input at this width), K cut to 96 -- three K steps, which the dispatcher's
    cost model still sends to the 96-wide tiles (225 tiles in one round of one workgroup per CU against 135 of 160 columns:
    10 + 0.82 * 0.6 * 3 < 0.95 * (10 + 0.82 * 3)).  Only the split-form layers under the range guard take this form."""
    cus = _cus()
    M, N, K = 1819, 1440, 96
    nb, nb3, nk = _cdiv(M, 128) * (N // 160), _cdiv(M, 128) * (N // 96), K // 32
    assert _not_short_input(M, N, cus) and _cdiv(M, 256) * (N // 160) < cus and 4 * nb > 2 * cus
    assert nb3 <= cus and nb <= cus and 10 + 0.82 * 0.6 * nk < 0.95 * (10 + 0.82 * nk)
    _check_exact(M, N, K, {}, lambda *run: 0, runs=[(1, 1, True), (2, 1, True)])


@pytest.mark.parametrize("C_", [160, 320])
def test_random_data_against_float64(C_):
    """random operands, N = K: relu layer with fp32 output and split-residual layer with split output under the guard, against
    float64 of the operands' values, bound 2e-5 * max(1, sqrt(K) / 8) (the project's dense-layer bound); two runs, same bits."""
    from tal_asrd_amd import ops, _native as N_
    lib = N_.lib()
    M = 256 * _cus() + 3
    N = K = C_
    g = torch.Generator().manual_seed(M + C_)
    x = torch.randn(M, K, generator=g).to(dev())
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev())
    b = torch.randn(N, generator=g).to(dev())
    xs, wsp = ops.split_f16x3(x), ops.split_f16x3(w)
    p = dict(xs=xs, ws=wsp, b=b, rs=xs)
    nws = max(int(lib.tal_linear_workspace_bytes(M, N, K)), 16)
    scratch = torch.empty(nws, dtype=torch.uint8, device=dev())
    pre = x.double() @ w.double().t() + b.double()
    bound = 2e-5 * max(1.0, K ** 0.5 / 8)
    for mode, out_split, guarded in [(1, 0, False), (2, 1, True)]:
        y1 = _launch(p, M, N, K, mode, out_split, guarded, scratch)[0].clone()
        y2 = _launch(p, M, N, K, mode, out_split, guarded, scratch)[0]
        assert torch.equal(y1, y2), (mode, "not repeatable")
        if out_split:
            h = y1.view(torch.float16).reshape(M, N // 32, 64).double()
            got = (h[:, :, :32] + h[:, :, 32:] / 2048.0).reshape(M, N)
            ref = x.double() + 0.5 * pre
        else:
            got = y1.double()
            ref = pre.clamp_min(0.0)
        err = float((got - ref).abs().max())
        print("dense 16x16x32, M=%d N=K=%d mode %d: max |err| vs float64 %.3e (bound %.3e)" % (M, K, mode, err, bound))
        assert err < bound, (mode, err)
