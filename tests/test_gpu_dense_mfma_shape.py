"""The fp16x3 dense layers on 16x16x32 MFMAs (csrc/gemm_w64.hip, the F16X3 branch of gemm_glds_kernel in csrc/gemm_f32.hip, the
16x16 staging write of csrc/gemm_common.h, the short-input kernel csrc/gemm_s64.hip) and the row split of csrc/gemm_plan.h, GPU.

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

The short-input kernel (64 x 80 and 32 x 80 tiles) and the row split (one round of 256 x 160 tiles, then a second launch for the
remaining rows) take their cases from tests/_dense_forms.py: every remainder of the K loop and the short prologue (K / 32 = 1 .. 9),
grids of every residue mod 8 with and without the magic division, both tile orders, last tiles of 1, 31 and 63 rows, N != K, and
every epilogue arm (fp32 / split residual; fp32 / guarded split / clamped split output) -- bit for bit against the model and
against the 128 x 160 kernels (option gemm_s64_below = 0); the row-split cases compare the whole output across the seam in two
scopes.  Their form is the restated plan of tests/_dense_forms.py (expect_plan), which tests/test_dense_forms_cpu.py holds to
csrc/gemm_plan.h; it is asserted before a case runs.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _dense_forms as F
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

PROF_GEMM = 0


def dev():
    return torch.device("cuda:0")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _cdiv(a, b):
    return -(-a // b)


_pack, _host_split, _int_operand = F.pack, F.host_split, F.int_operand


def _exact_problem(M, N, K):
    """the exact integer model (tests/_dense_forms.py: exact_model, numpy on the host) with its operands on the device: x, w and
    the residual in the split format, the bias, and the residual once more as a plain fp32 matrix (rh + rl / 2048, exact)"""
    m = F.exact_model(M, N, K)
    d = dev()
    u8 = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1)).to(d)
    p = dict(xs=u8(_pack(m["xh"], m["xl"])), ws=u8(_pack(m["wh"], m["wl"])), b=torch.from_numpy(m["b"]).to(d), rf=torch.from_numpy(m["rf"]).to(d),
             exp=m["exp"])
    if N % 32 == 0:                          # (no split form of an [M, N] matrix otherwise: fp32 in and out only)
        p["rs"] = u8(_pack(m["rh"], m["rl"]))
    return p


_PROBLEMS = {}


def _problem(M, N, K):
    key = (M, N, K)
    if key not in _PROBLEMS:
        _PROBLEMS.clear()                    # (one at a time: the large ones are 100 MB on the device)
        _PROBLEMS[key] = _exact_problem(M, N, K)
    return _PROBLEMS[key]


GUARD = 5


def _launch(p, M, N, K, mode, out_split, guarded, scratch, res_form=None):
    """one dense layer; returns (output rows, floats of the split-K scratch that were written, profiling scopes, their work).
    res_form of a mode-2 layer: "split" (guarded call only) or "f32"; default: split under the guard, fp32 without it (the
    unguarded entry point takes no other)"""
    from tal_asrd_amd import _native as N_
    lib = N_.lib()
    d = dev()
    if out_split:
        ybuf = torch.full(((M + GUARD) * N * 4,), 0x5A, dtype=torch.uint8, device=d)
    else:
        ybuf = torch.full((M + GUARD, N), 4321.0, device=d)
    scratch.fill_(0xFF)                      # NaN as fp32; a K slice writes whole tiles of finite partial sums
    flag = torch.zeros(16, dtype=torch.int32, device=d)
    res, res_split = None, 0
    if mode == 2:
        res_split = int((res_form or ("split" if guarded else "f32")) == "split")
        assert guarded or not res_split
        res = p["rs"] if res_split else p["rf"]
    lib.tal_prof_reset()
    lib.tal_prof_enable(1)
    try:
        if guarded:
            N_.check(lib.tal_linear_f16x3_guarded_fwd(N_.ptr(p["xs"]), N_.ptr(p["ws"]), N_.ptr(p["b"]), N_.ptr(res), res_split, 0.5, mode, M, N, K,
                                                      N_.ptr(ybuf), out_split, N_.ptr(flag), N_.ptr(scratch), scratch.numel(), N_.stream_handle()),
                     "tal_linear_f16x3_guarded_fwd")
        else:
            N_.check(lib.tal_linear_f16x3_fwd(N_.ptr(p["xs"]), N_.ptr(p["ws"]), N_.ptr(p["b"]), N_.ptr(res), 0.5, mode, M, N, K, N_.ptr(ybuf), out_split,
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


def _where(bad):
    """rows and columns of a mismatch, for the message (the integer model tells which rows / columns are off)"""
    r, c = np.nonzero(bad)
    return "%d elements off; rows %s, columns %s" % (len(r), np.unique(r)[:12].tolist(), np.unique(c)[:12].tolist())


def _check_exact(M, N, K, options, expect_written, runs=RUNS, scopes=1):
    """every run bit for bit against the model, in `scopes` dense launch scopes whose work adds up to the call's.  A run is
    (mode, split output, guarded call) or (mode, split output, guarded call, residual form)."""
    from tal_asrd_amd import _native as N_
    lib = N_.lib()
    p = _problem(M, N, K)
    nws = max(int(lib.tal_linear_workspace_bytes(M, N, K)), 16)
    scratch = torch.empty(nws, dtype=torch.uint8, device=dev())
    try:
        for name, value in options.items():
            N_.set_option(name, value)
        for run in runs:
            mode, out_split, guarded = run[:3]
            what = (M, N, K, options) + tuple(run)
            y, written, nscopes, work = _launch(p, M, N, K, mode, out_split, guarded, scratch, *run[3:])
            assert nscopes == scopes and work == 2.0 * M * N * K, ("dense launch scopes and their whole work", what, nscopes, work)
            assert written == expect_written(mode, out_split, guarded), ("split-K scratch floats written", what, written)
            if out_split:
                got = y.cpu().numpy().view(np.uint16).reshape(M, -1)
                want = _host_split(p["exp"][mode]).view(np.uint16).reshape(M, -1)
                assert np.array_equal(got, want), (what, _where((got != want).reshape(M, N // 32, 2, 32).any(axis=2).reshape(M, N)))
            else:
                got, want = y.cpu(), torch.from_numpy(p["exp"][mode])
                assert torch.equal(got, want), (what, _where((got != want).numpy()))
    finally:
        for name in options:
            N_.set_option(name, F.OPTION_DEFAULTS.get(name, 0))


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


# ---- the short-input kernel (gemm_s64_kernel, csrc/gemm_s64.hip) and the row split of gemm_plan ----------------------------------------
# The cases and the form each is there for: tests/_dense_forms.py.  Which form ran: expect_plan restates the plan (held to
# csrc/gemm_plan.h in tests/test_dense_forms_cpu.py) and is asserted first, with the CU count of the device, so that a case that left
# its arm fails loudly; on the device a 64 x 80 launch is one scope with the whole work and no scratch, a row split two scopes.

# One test per table, not one per case (the suite's GPU test count stays close to what it was): a test walks every case, goes on
# after a case that fails its assertions and names every failed case at the end; any other error ends it at once.

def _walk(cases, check):
    failed = []
    for case in cases:
        try:
            check(case)
        except AssertionError as e:
            failed.append("%s: %s" % (case["id"], " ".join(str(e).split())[:400]))
    assert not failed, "%d of %d cases failed:\n%s" % (len(failed), len(cases), "\n".join(failed))


def test_exact_s64():
    """every case of short_cases: one launch of gemm_s64_kernel in every epilogue arm (fp32 / split residual, fp32 / guarded split /
    clamped split output), bit for bit against the integer model; then the same runs with option gemm_s64_below = 0 -- the
    128 x 160 kernels, which the model is exact for in any summation order -- must give the same bits.  The gemm_s64_rows /
    gemm_s64_order variants of a shape are compared with the same expected bits, hence with the default run."""
    cus = _cus()

    def check(case):
        F.check_short_form(case, cus)
        M, N, K = case["M"], case["N"], case["K"]
        runs = F.runs_of(case)
        _check_exact(M, N, K, case["options"], lambda *run: 0, runs=runs)
        _check_exact(M, N, K, dict(case["options"], gemm_s64_below=0), lambda *run: 0, runs=runs)

    _walk(F.short_cases(cus), check)


def test_exact_row_split():
    """every case of row_split_cases: one round of 256 x 160 tiles and a second launch (32 x 80, 64 x 80 or 128 x 160 tiles) for the
    remaining rows, which starts at row rows1 with every pointer moved on: the WHOLE output against the integer model, the rows on
    both sides of the seam and the last row included.  Two scopes whose work adds up to the call's; no scratch."""
    cus = _cus()

    def check(case):
        first, second = F.expect_plan(case, cus)
        assert first[0] == "w64" and second[0] == case["second"][0] and second[2] == first[1]
        _check_exact(case["M"], case["N"], case["K"], {}, lambda *run: 0, runs=F.ROW_SPLIT_RUNS, scopes=2)

    _walk(F.row_split_cases(cus), check)          # (row_split_cases asserts the plan's conditions at this CU count)


RANDOM_S64 = [(300, 640, 896), (300, 896, 640), (700, 1152, 64), (129, 160, 96), (300, 880, 640), (700, 1120, 64)]


def test_random_data_s64_against_float64():
    """short inputs on random operands at N != K and K / 32 = 28, 20, 2 and 3 (remainders of 0, 2 and 3 K steps of gemm_s64_kernel;
    the project's widths give 1 and 3 only): operands from ops.split_f16x3, outputs against float64 of the operands' decoded values,
    bound 2e-5 * max(1, sqrt(K) / 8) (the project's dense-layer bound); two runs, same bits.
    gemm_s64_kernel takes N % 80 == 0 only (gemm_s64_ok): N = 896 and 1152 -- the widths of SDModel(n_mels=64) -- are no
    multiples of 80 and run on 128 x 160 tiles with a column tail; 880 and 1120 stand in for them on the 64 x 80 tiles at the same K.
    Measured max |err| per shape: profiles/dense_mfma_shape.txt section 6."""
    _walk([dict(id="%dx%dx%d" % s, shape=s) for s in RANDOM_S64], lambda case: _random_s64(*case["shape"]))


def _random_s64(M, N, K):
    from tal_asrd_amd import ops, _native as N_
    lib = N_.lib()
    cus = _cus()
    if N % 80 == 0:
        assert F.expect_plan(dict(M=M, N=N, K=K), cus)[0][0] == "s64", "no short input at %d CUs" % cus
    g = torch.Generator().manual_seed(1000 * M + N + K)
    x = torch.randn(M, K, generator=g).to(dev())
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev())
    b = torch.randn(N, generator=g).to(dev())
    r = torch.randn(M, N, generator=g).to(dev())
    dec = lambda s, rows: (lambda h: (h[:, :, :32] + h[:, :, 32:] / 2048.0).reshape(rows, -1))(s.view(torch.float16).reshape(rows, -1, 64).double())
    xs, wsp = ops.split_f16x3(x), ops.split_f16x3(w)
    p = dict(xs=xs, ws=wsp, b=b, rf=r)
    runs = [(1, 0, False, None), (2, 0, False, "f32")]
    if N % 160 == 0:
        p["rs"] = ops.split_f16x3(r)
        runs.append((2, 1, True, "split"))
    scratch = torch.empty(max(int(lib.tal_linear_workspace_bytes(M, N, K)), 16), dtype=torch.uint8, device=dev())
    pre = dec(xs, M) @ dec(wsp, N).t() + b.double()
    bound = 2e-5 * max(1.0, K ** 0.5 / 8)
    for mode, out_split, guarded, res_form in runs:
        y1, _, scopes, work = _launch(p, M, N, K, mode, out_split, guarded, scratch, res_form)
        y1 = y1.clone()
        y2 = _launch(p, M, N, K, mode, out_split, guarded, scratch, res_form)[0]
        assert scopes == 1 and work == 2.0 * M * N * K
        assert torch.equal(y1, y2), (mode, "not repeatable")
        got = dec(y1, M) if out_split else y1.double()
        ref = pre.clamp_min(0.0) if mode == 1 else (dec(p["rs"], M) if res_form == "split" else r.double()) + 0.5 * pre
        err = float((got - ref).abs().max())
        print("dense %s, M=%d N=%d K=%d mode %d out_split %d res %s: max |err| vs float64 %.3e (bound %.3e)" % (
            "64 x 80" if N % 80 == 0 else "128 x 160", M, N, K, mode, out_split, res_form, err, bound))
        assert err < bound, (mode, out_split, err)
