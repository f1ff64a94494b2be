"""The fp16x3 window at every site that makes fp16 halves (GPU): top of the range (the status word fires exactly when it must),
non-finite input (flag raised OR the non-finite value is in the output -- never finite output under a clear flag), and the
bottom of the range (magnitude sweeps against float64 with a tolerance derived from host float32, never from the kernels).
The format itself is restated in tests/_fp16x3_ref.py and tied down on the CPU in tests/test_fp16x3_ref_cpu.py.

SITES accounts for every `note_range(`, `split_f16x3(` and `split_f16x3_pair(` call under tal_asrd_amd/csrc (counts per
function; tests/test_fp16x3_ref_cpu.py::test_site_table_accounts_for_every_converting_call re-derives them from the sources).
`reach` is the public call and shape that takes the branch, `test` the case below that covers it ("-" with the reason where
no case does).  Measured errors per family and sweep point next to the host float32 error: profiles/fp16x3_range.txt.

Tolerance of the sweeps (from the reference's own error and the format, never from what the kernels give): |got - want| <= max(4 * e32, f) [+ 2^-22 |want| where the
output itself is stored in the split form: 22 mantissa bits], e32 = max error of the same operation in host float32 against
the same float64 reference, f = K * 2^-35 * max|other operand| (include/tal_asrd.h: a value below 2^-24 loses its low half)."""
import numpy as np
import pytest
import torch

from tests import _fp16x3_ref as R
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

# (file, function, {call: count}, guard, reach, test)
SITES = [
    ("gemm_f32.hip", "split_f16x3_kernel", {"note_range": 1, "split_f16x3": 1}, "guarded inside tal_tds_fwd, clamped",
     "tal_split_f16x3_fwd (no flag); tal_tds_fwd with option tds_fp32_activations (flag)", "test_split_pass_bit_exact_on_every_pattern, test_dense_and_split_pass_sweep, test_tds_sites[fp32_activations-s*.conv]"),
    ("gemm_f32.hip", "gemm_splitk_fixup_kernel", {"note_range": 1, "split_f16x3": 1}, "guarded, clamped",
     "tal_linear_f16x3_guarded_fwd 13057 x 800: K-sliced tail tile of the 256 x 160 kernel", "test_dense_guard[w64_tail]"),
    ("gemm_common.h", "gemm_epilogue", {"note_range": 1, "split_f16x3_pair": 2, "split_f16x3": 1}, "guarded arm (pair) and unguarded arm (clamped)",
     "tal_linear_f16x3_guarded_fwd 3300 x 800 mode 2 with an fp32 residual / mode 0; tal_linear_f16x3_fwd out_split (no flag)",
     "test_dense_guard[shared_f32res], test_dense_guard[shared_mode0], test_dense_unguarded_arm_clamps"),
    ("gemm_common.h", "gemm_epilogue_split", {"note_range": 1, "split_f16x3_pair": 2}, "guarded",
     "tal_linear_f16x3_guarded_fwd 3300 x 800 (128 x 160), 1819 x 1440 (128 x 96), 13057 x 800 (256 x 160, gemm_w64.hip)",
     "test_dense_guard[glds160], [glds96], [w64_tail], [w64_rowsplit]"),
    ("gemm_s64.hip", "gemm_s64_kernel", {"note_range": 1, "split_f16x3_pair": 2, "split_f16x3": 1}, "guarded (row_ok mask) and unguarded arm",
     "tal_linear_f16x3_guarded_fwd 1500 x 800 (64 rows), 129 x 800 (32 rows), remainder launch of 13185 x 800",
     "test_dense_guard[s64], [s64_half], [w64_rowsplit]; values bit for bit in both arms: test_exact_s64, test_exact_row_split "
     "(tests/test_gpu_dense_mfma_shape.py)"),
    ("gconv.hip", "gconv_s2_c1_kernel", {"note_range": 1, "split_f16x3": 1}, "guarded, clamped",
     "tal_tds_fwd, first resize conv of an all-split stage", "test_tds_sites[split-s0.down]"),
    ("gconv.hip", "gconv_mfma_kernel", {"note_range": 3, "split_f16x3": 10, "split_f16x3_pair": 4}, "guarded (pair) / unguarded (clamped)",
     "tal_tds_fwd: stride-1 epilogue 10 / 14 channels (s0.conv, s1.conv), stride-2 epilogue (s1.down, s2.down); slab fill from fp32 "
     "input: tal_gconv_*_f16x3_fwd (no flag) and tal_tds_fwd with option tds_fp32_activations (flag); fused resize + block conv: "
     "option gconv_c1_fuse; long tiles: option gconv_short_below = 0",
     "test_tds_sites[split-s0.conv], [split-s1.down], [split-s1.conv], [split-s2.down], [split_long_tiles-*]; slab fill: "
     "[fp32_activations-s*.down], [fp32_activations-s*.fc3]; fused: [c1_fused-s0.down], [c1_fused-s0.conv]; sweeps "
     "test_block_conv_sweep / test_resize_conv_sweep"),
    ("gconv.hip", "gconv18_shift_kernel", {"note_range": 1, "split_f16x3": 8, "split_f16x3_pair": 4}, "guarded (pair) / unguarded (clamped)",
     "tal_tds_fwd third stage (18 channels per group, split in / out)", "test_tds_sites[split-s2.conv], [split_long_tiles-s2.conv]"),
    ("gconv.hip", "pack_gconv_shift18_kernel", {"split_f16x3": 1}, "weights: the caller checks the range at pack time",
     "tal_pack_gconv_f16x3_weight", "- weight side (test_fp16_range_guard_routes_to_exact_kernels covers the pack-time check)"),
    ("gconv.hip", "pack_gconv_mfma_kernel", {"split_f16x3": 1}, "weights: the caller checks the range at pack time",
     "tal_pack_gconv_f16x3_weight", "- weight side, as above; test_block_conv_sweep scales the weights through it"),
    ("head.hip", "head_argmax_kernel", {"split_f16x3": 2, "note_range": 1}, "guarded on the device: the fp32 kernel redoes the call",
     "tal_sd_head_fwd ids-only, 3000 x 128 -> 6008", "test_head_out_of_range, test_head_sweep"),
]
# launch_split_f16x3 callers (api.hip): tal_split_f16x3_fwd (no flag), tds_fwd_impl (flag), sd_head_after_feat (flag: test_head_out_of_range)


def dev():
    return torch.device("cuda:0")


def _lib():
    from tal_asrd_amd import _native as N_
    return N_, N_.lib()


def _gpu_split(x):
    from tal_asrd_amd import ops
    return ops.split_f16x3(torch.as_tensor(x, dtype=torch.float32).contiguous().to(dev()))


def _host_split_bytes(x, clamped=True):
    """split form of a host array built by the NumPy reference (for planting values the clamped split pass would clamp)"""
    hi, lo = (R.split_clamped if clamped else R.split_plain)(x)
    return torch.from_numpy(R.pack_rows(hi, lo).view(np.uint8).reshape(-1).copy()).to(dev())


def _decode(buf, rows, C):
    return R.decode_rows(buf.cpu().numpy().view(np.uint16)[:rows * C * 2], rows, C)


# ------------------------------------------------------------------------------------------------ split pass, bit for bit
def test_split_pass_bit_exact_on_every_pattern():
    """tal_split_f16x3_fwd against the NumPy restatement over +-0, fp32 subnormals, the fp16 subnormal range, rounding midpoints
    near 1 and near 65504, 65504 .. 65536, +-Inf, NaN: identical bytes (NaN halves compared as NaN)."""
    v = R.interesting_f32_patterns()
    K = 32
    rows = v.size // K
    got = _gpu_split(v.reshape(rows, K)).cpu().numpy().view(np.uint16)
    ghi, glo = R.unpack_rows(got, rows, K)
    whi, wlo = R.split_clamped(v.reshape(rows, K))
    for name, g, w in (("hi", ghi, whi), ("lo", glo, wlo)):
        gb, wb = g.view(np.uint16), w.view(np.uint16)
        same = (gb == wb) | (np.isnan(g) & np.isnan(w))
        bad = np.argwhere(~same)
        assert bad.size == 0, "%s halves differ at %d patterns, first: x=%r got=%r want=%r" % (
            name, len(bad), v.reshape(rows, K)[tuple(bad[0])], g[tuple(bad[0])], w[tuple(bad[0])])
    # the table of tests/_fp16x3_ref.py, clamped column
    xs = np.array([r[0] for r in R.NONFINITE_TABLE] + [1.0] * (32 - len(R.NONFINITE_TABLE)), dtype=np.float32).reshape(1, 32)
    hi, lo = R.unpack_rows(_gpu_split(xs).cpu().numpy().view(np.uint16), 1, 32)
    for i, (x, (h, l), _, _) in enumerate(R.NONFINITE_TABLE):
        assert float(hi[0, i]) == h and float(lo[0, i]) == l, (x, float(hi[0, i]), float(lo[0, i]))


# ------------------------------------------------------------------------------------------------ dense layers, C ABI
def _guarded(lib, N_, xs, ws_, b, res, res_split, alpha, mode, M, N, K, out_split, flag, guard_rows=2):
    y = torch.full(((M + guard_rows) * N * 4,), 0x5A, dtype=torch.uint8, device=dev())
    nws = lib.tal_linear_workspace_bytes(M, N, K)
    wsb = torch.empty(max(nws, 16), dtype=torch.uint8, device=dev())
    N_.check(lib.tal_linear_f16x3_guarded_fwd(N_.ptr(xs), N_.ptr(ws_), N_.ptr(b), N_.ptr(res) if res is not None else None, res_split, alpha,
                                              mode, M, N, K, N_.ptr(y), out_split, N_.ptr(flag) if flag is not None else None,
                                              N_.ptr(wsb), nws, N_.stream_handle()), "tal_linear_f16x3_guarded_fwd")
    torch.cuda.synchronize()
    assert bool((y[M * N * 4:] == 0x5A).all()), "wrote behind the output"
    return y


# name -> (C, M, mode, res_split, rows to plant in).  Row counts from the dispatcher (csrc/gemm_f32.hip launch_gemm, 256 CUs).
DENSE = {
    "s64":          (800, 1500, (1, 2), 1, "0 last mid"),           # 64 x 80 tiles, whole tiles only: rows 1472.. sit in a partial tile
    "s64_half":     (800, 129, (1, 2), 1, "0 last"),                # 32-row tiles; row 128 alone in the last tile
    "glds160":      (800, 3300, (1, 2), 1, "0 last mid"),           # 128 x 160 tiles, static-addressing epilogue
    "glds96":       (1440, 1819, (1, 2), 1, "0 last mid"),          # 128 x 96 tiles
    "w64_tail":     (800, 13057, (1, 2), 1, "0 13055 last"),        # 256 x 160 round + K-sliced tail tiles (row 13056: fix-up kernel)
    "w64_rowsplit": (800, 13185, (1, 2), 1, "0 13055 13056 last"),  # 256 x 160 round on 13056 rows + a short-input launch for 129
    "shared_f32res": (800, 3300, (2,), 0, "0 last mid"),            # fp32 residual: the shared epilogue's guarded arm
    "shared_mode0": (800, 3300, (0,), 0, "0 last"),                 # mode 0 with a split output: shared epilogue
}
# value the planted output element takes -> must the flag rise?   (65505 .. 65519 round to 65504 in fp16 but are out of range)
TOP = [(6.0e4, False), (65504.0, False), (65505.0, True), (65519.0, True), (65520.0, True), (1.0e5, True),
       (float("inf"), True), (float("-inf"), True), (float("nan"), True)]


def _rows_of(spec, M):
    return [{"0": 0, "last": M - 1, "mid": M // 2 + 1}.get(t, int(t) if t.isdigit() else None) for t in spec.split()]


@pytest.mark.parametrize("name", list(DENSE))
def test_dense_guard(name):
    """One output element of a guarded fp16x3 dense layer is steered to a chosen value while every other converted value stays
    O(1): relu / plain layers through one x element under a one-hot weight row (y = 2 x, exact), residual layers through one
    residual element plus alpha * bias (65504 + 1, ... exact); Inf / NaN come in through the bias (a split operand cannot
    hold them) or the residual.  First row, last valid row (a partial tile), rows of the tail / remainder launch, first and
    last column block.  Finite values: the flag rises exactly beyond 65504; at 6e4 and 65504 the planted value arrives
    exactly and (first position) the whole output matches float64.  Non-finite values: flag raised or the value is in the
    output.  NaN under relu is not planted: relu is fmaxf(v, 0) in every kernel, fp32 ones included, and maps NaN to 0
    (include/tal_asrd.h says so)."""
    N_, lib = _lib()
    C, M, modes, res_split, rowspec = DENSE[name]
    g = torch.Generator().manual_seed(C + M)
    x0 = torch.randn(M, C, generator=g).numpy()
    w0 = (torch.randn(C, C, generator=g) / C ** 0.5).numpy()
    b0 = torch.randn(C, generator=g).numpy()
    r0 = torch.randn(M, C, generator=g).numpy()
    alpha = 0.5
    xs_base = _host_split_bytes(x0)
    rs_base = _host_split_bytes(r0) if res_split else None
    rows = _rows_of(rowspec, M)
    row_bytes = C * 4
    for mode in modes:
        for i, row in enumerate(rows):
            col, kcol = ((5, 17), (C - 1, C - 3))[(i + 1) % 2]          # the last row sits in the last column block
            w = w0.copy()
            w[col, :] = 0.0
            if mode != 2:
                w[col, kcol] = 2.0
            wsp = _gpu_split(w)
            for val, must in TOP:
                finite = bool(np.isfinite(val))
                if mode == 1 and (np.isnan(val) or val < 0):
                    continue                                   # relu(-inf) = 0 and relu(NaN) = fmaxf(NaN, 0) = 0: nothing to convert
                x, b, res = x0[row:row + 1].copy(), b0.copy(), r0[row:row + 1].copy()
                b[col] = 0.0
                if mode == 2:
                    # y[row, col] = res + alpha * bias: 65504 + 0.5 * 2 = 65505 exactly, ...
                    base = min(val, 65504.0) if finite else val
                    res[0, col] = base
                    b[col] = (val - base) / alpha if finite else 0.0
                elif finite:
                    x[0, kcol] = val / 2.0                     # y[row, col] = 2 x: exact in the fp16x3 form
                else:
                    x[0, kcol] = 1.0
                    b[col] = val
                xs = xs_base.clone()
                xs[row * row_bytes:(row + 1) * row_bytes] = _host_split_bytes(x)
                rs = None
                if mode == 2 and res_split:
                    rs = rs_base.clone()
                    # (a non-finite residual in the split form: unclamped halves, as a guarded kernel upstream writes them)
                    rs[row * row_bytes:(row + 1) * row_bytes] = _host_split_bytes(res, clamped=False)
                elif mode == 2:
                    rfull = r0.copy()
                    rfull[row] = res[0]
                    rs = torch.from_numpy(rfull).to(dev())
                flag = torch.zeros(16, dtype=torch.int32, device=dev())
                y = _guarded(lib, N_, xs, wsp, torch.from_numpy(b).to(dev()), rs, res_split if mode == 2 else 0, alpha, mode, M, C, C, 1, flag)
                what = (name, mode, row, col, val)
                raised = int(flag[0]) != 0
                assert int(flag[1:].abs().sum()) == 0, what
                got_rc = _decode(y[row * row_bytes:(row + 1) * row_bytes], 1, C)[0, col]
                if not finite:
                    assert raised or not np.isfinite(got_rc), ("finite output under a clear flag", what, got_rc)
                    continue
                assert raised == must, ("flag", what, raised)
                if must:
                    continue
                assert got_rc == val, (what, got_rc)                    # the planted value arrives exactly
                if i == 0:
                    got = _decode(y, M, C)
                    xfull = x0.copy(); xfull[row] = x[0]
                    rfull = r0.copy(); rfull[row] = res[0]
                    xd = R.decode(*R.split_clamped(xfull))
                    rd = R.decode(*R.split_clamped(rfull)) if res_split else rfull.astype(np.float64)
                    acc = xd @ w.astype(np.float64).T + b
                    want = np.maximum(acc, 0) if mode == 1 else (rd + alpha * acc if mode == 2 else acc)
                    a32 = (torch.from_numpy(xd.astype(np.float32)) @ torch.from_numpy(w).t() + torch.from_numpy(b)).numpy()
                    h32 = np.maximum(a32, 0) if mode == 1 else (rd.astype(np.float32) + np.float32(alpha) * a32 if mode == 2 else a32)
                    e32 = float(np.abs(h32.astype(np.float64) - want).max())
                    err = np.abs(got - want)
                    assert bool((err <= 4 * e32 + 2.0 ** -22 * np.abs(want)).all()), ("accuracy", what, float(err.max()), e32)


def test_dense_unguarded_arm_clamps():
    """tal_linear_f16x3_fwd with a split output has no status word: its halves are clamped (documented), so a value beyond the
    range arrives as 65504 + 65504 / 2048, finite, and in-range values match float64."""
    N_, lib = _lib()
    C, M = 800, 3300
    g = torch.Generator().manual_seed(9)
    x = torch.randn(M, C, generator=g).numpy(); w = (torch.randn(C, C, generator=g) / C ** 0.5).numpy(); b = torch.randn(C, generator=g).numpy()
    w[5, :] = 0.0; w[5, 17] = 2.0; b[5] = 0.0; x[0, 17] = 5.0e4
    y = _guarded(lib, N_, _host_split_bytes(x), _gpu_split(w), torch.from_numpy(b).to(dev()), None, 0, 0.0, 1, M, C, C, 1, None)
    got = _decode(y, M, C)
    assert got[0, 5] == 65504.0 + 65504.0 / 2048.0
    xd = R.decode(*R.split_clamped(x))
    want = np.maximum(xd @ w.astype(np.float64).T + b, 0)
    want[0, 5] = got[0, 5]
    d32 = np.abs(np.maximum((torch.from_numpy(xd.astype(np.float32)) @ torch.from_numpy(w).t() + torch.from_numpy(b)).numpy(), 0) - want)
    d32[0, 5] = 0.0
    e32 = float(d32.max())
    assert bool((np.abs(got - want) <= 4 * e32 + 2.0 ** -22 * np.abs(want)).all())


# ------------------------------------------------------------------------------------------------ magnitude sweeps
def _record(family, case, err, e32, f, scale):
    line = "%-12s %-22s err %.3e  e32 %.3e  f %.3e  scale %.3e  err/scale %.3e  allowed/scale %.3e" % (
        family, case, err, e32, f, scale, err / scale if scale else 0.0, max(4 * e32, f) / scale if scale else 0.0)
    print(line)


def _sweep_cases():
    for p in R.SWEEP_EXPONENTS:
        yield "x*2^%d" % p, p, 0, False
    for q in R.SWEEP_EXPONENTS:
        if q != 0:
            yield "w*2^%d" % q, 0, q, False
    yield "mixed 2^-30..2^10", 0, 0, True


def _mixed_scale(C, rng):
    return (2.0 ** rng.integers(-30, 11, size=C)).astype(np.float32)


def test_dense_and_split_pass_sweep():
    """x -> tal_split_f16x3_fwd -> tal_linear_f16x3_fwd (fp32 output) against float64 of the ORIGINAL fp32 operands, operands
    scaled over 2^-40 .. 2^14 and one case with columns of x spanning 2^-30 .. 2^10 in a row: the split pass and the dense
    kernel's MFMA inputs must keep fp16 subnormals (a flush would cost 2^-20 relative at 2^-5)."""
    N_, lib = _lib()
    M, C = 600, 800
    rng = np.random.default_rng(77)
    x0 = R.clipped_randn(rng, (M, C)); w0 = (R.clipped_randn(rng, (C, C)) / np.float32(C ** 0.5)).astype(np.float32)
    mix = _mixed_scale(C, rng)
    fails = []
    for case, p, q, mixed in _sweep_cases():
        x = (x0 * np.float32(2.0 ** p)) * (mix if mixed else np.float32(1)); w = w0 * np.float32(2.0 ** q)
        x = x.astype(np.float32); w = w.astype(np.float32)
        y = torch.full(((M + 2) * C,), 7.0, dtype=torch.float32, device=dev())
        nws = lib.tal_linear_workspace_bytes(M, C, C)
        wsb = torch.empty(max(nws, 16), dtype=torch.uint8, device=dev())
        xs, wsp = _gpu_split(x), _gpu_split(w)
        N_.check(lib.tal_linear_f16x3_fwd(N_.ptr(xs), N_.ptr(wsp), None, None, 0.0, 0, M, C, C, N_.ptr(y), 0, N_.ptr(wsb), nws,
                                          N_.stream_handle()), "tal_linear_f16x3_fwd")
        torch.cuda.synchronize()
        assert bool((y[M * C:] == 7.0).all())
        got = y[:M * C].reshape(M, C).cpu().double().numpy()
        want = x.astype(np.float64) @ w.astype(np.float64).T
        e32 = float(np.abs((torch.from_numpy(x) @ torch.from_numpy(w).t()).double().numpy() - want).max())
        f = C * 2.0 ** -35 * max(float(np.abs(w).max()) if p < 0 or mixed else 0.0, float(np.abs(x).max()) if q < 0 else 0.0)
        err = float(np.abs(got - want).max())
        _record("dense+split", case, err, e32, f, float(np.abs(want).max()))
        if not err <= max(4 * e32, f):
            fails.append((case, err, e32, f))
    assert not fails, fails


def _conv_sweep(family, cig, cog, stride):
    from tal_asrd_amd import ops
    G, B, T = 80, 2, 300
    rng = np.random.default_rng(1000 * cig + cog)
    x0 = R.clipped_randn(rng, (B, T, G * cig)); w0 = (R.clipped_randn(rng, (G * cog, cig, 21)) / np.float32((21 * cig) ** 0.5)).astype(np.float32)
    mix = _mixed_scale(G * cig, rng)
    zero_b = torch.zeros(G * cog, device=dev())
    fails = []
    for case, p, q, mixed in _sweep_cases():
        x = (x0 * np.float32(2.0 ** p)).astype(np.float32); w = (w0 * np.float32(2.0 ** q)).astype(np.float32)
        if mixed:
            x = (x * mix).astype(np.float32)
        alpha = float(2.0 ** -q)             # stride 1: y = x + alpha relu(conv): the conv term stays at the scale of x
        xt, wt = torch.from_numpy(x), torch.from_numpy(w)
        wf = ops.pack_gconv_f16x3_weight(wt.to(dev()), G, stride=stride)

        def ref(dt):
            c = torch.nn.functional.conv1d(xt.to(dt).permute(0, 2, 1), wt.to(dt), None, stride=stride, padding=10 if stride == 1 else 0, groups=G)
            return (xt.to(dt).permute(0, 2, 1) + alpha * torch.relu(c) if stride == 1 else c).permute(0, 2, 1).double().numpy()
        if stride == 1:
            got = ops.gconv_res_f16x3(xt.to(dev()), wf, zero_b, alpha, G)
        else:
            got = ops.gconv_s2_f16x3(xt.to(dev()), wf, zero_b, G * cog, G)
        torch.cuda.synchronize()
        want = ref(torch.float64)
        e32 = float(np.abs(ref(torch.float32) - want).max())
        K = 21 * cig
        f = K * 2.0 ** -35 * max(float(np.abs(w).max()) if p < 0 or mixed else 0.0, float(np.abs(x).max()) if q < 0 else 0.0) * (alpha if stride == 1 else 1.0)
        err = float(np.abs(got.cpu().double().numpy() - want).max())
        _record(family, "%d->%d %s" % (cig, cog, case), err, e32, f, float(np.abs(want).max()))
        if not err <= max(4 * e32, f):
            fails.append((case, err, e32, f))
    assert not fails, fails


@pytest.mark.parametrize("cg", [10, 18])
def test_block_conv_sweep(cg):
    """TDSBlock conv on the matrix cores (fp32 in / out: slab fill from fp32 input, weight fragments), magnitude sweep."""
    _conv_sweep("block conv", cg, cg, 1)


def test_resize_conv_sweep():
    """stride-2 resize conv 10 -> 14 channels per group on the matrix cores, magnitude sweep."""
    _conv_sweep("resize conv", 10, 14, 2)


# ------------------------------------------------------------------------------------------------ the head
def _head_ids(feat, wl, bl, form):
    """ids-only head on features given exactly: the embedding layer is the identity (128 -> 128, one exact product per output).
    form: 'long' (A-stationary arg-max kernel), 'fused' (dense layer's arg-max epilogue, option head_no_astationary),
    'split' (tal_sd_head_split_fwd: features arrive in the split form, 22 bits)."""
    from tal_asrd_amd import ops, _native as N_
    eye = torch.eye(R.HEAD_E, device=dev())
    zb = torch.zeros(R.HEAD_E, device=dev())
    x = torch.from_numpy(feat).to(dev())
    wl_d, bl_d = torch.from_numpy(wl).to(dev()), torch.from_numpy(bl).to(dev())
    if form == "fused":
        N_.set_option("head_no_astationary", 1)
    try:
        if form == "split":
            # (the embedding layer is 4 * identity on x = feat / 4, both exact: features beyond the fp16 range can then arrive
            #  from split operands that are inside it)
            f, _, ids = ops.sd_head(_gpu_split(x * 0.25).view(torch.float32).reshape(feat.shape), eye, zb, wl_d, bl_d, want_logits=False,
                                    want_ids=True, x_split=True, w_embed_split=_gpu_split(eye * 4.0))
        else:
            f, _, ids = ops.sd_head(x, eye, zb, wl_d, bl_d, want_logits=False, want_ids=True)
        torch.cuda.synchronize()
    finally:
        if form == "fused":
            N_.set_option("head_no_astationary", 0)
    return f.cpu().numpy(), ids.cpu().numpy().astype(np.int64)


def _check_ids(feat_out, ids, wl, bl, what, max_skip=0.01):
    want, arg, keep, e32 = R.head_reference(feat_out, wl, bl)
    all_nan = np.isnan(want).all(axis=1)
    skipped = float((~all_nan & ~keep).mean())
    print("head %s: e32 %.3e, rows inside the margin %.4f, all-NaN rows %d" % (what, e32, skipped, int(all_nan.sum())))
    assert skipped <= max_skip, (what, skipped)
    bad = keep & (ids != arg)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].ravel().tolist())
    return skipped


@pytest.mark.parametrize("form", ["long", "fused", "split"])
def test_head_sweep(form):
    """speaker ids against the float64 arg-max with the features scaled by 2^p over the sweep (reference: float64 logits from
    the call's own fp32 `feat` output; rows whose float64 top-2 margin is within 8 * e32 are skipped, at most 1 % of them)."""
    for p in R.SWEEP_EXPONENTS:
        feat, wl, bl = R.head_case(p)
        f, ids = _head_ids(feat, wl, bl, form)
        if form != "split":
            assert np.array_equal(f, feat)
        _check_ids(f, ids, wl, bl, "%s 2^%d" % (form, p))


# (a NaN feature cannot be handed to the split form through the clamped split pass: that one combination is not a case)
HEAD_CASES = [(form, what) for form in ("long", "fused", "split")
              for what in ("weight", "inf_weight", "nan_weight", "feature", "feature_65519", "bias", "nan_row") if (form, what) != ("split", "nan_row")]


@pytest.mark.parametrize("form,what", HEAD_CASES)
def test_head_out_of_range(form, what):
    """One logit weight / one feature / one logit bias beyond 65504, an Inf and a NaN logit weight, NaN in one feature row, on
    all three forms: the ids must equal the float64 arg-max of the fp32 operands on every row outside the margin (a NaN logit
    never wins, as in every arg-max of the library).  Each case is built so that clamped halves would change the winner."""
    feat, wl, bl = R.head_case(0)
    feat, wl, bl = feat.copy(), wl.copy(), bl.copy()
    row = R.HEAD_M - 7
    if what == "weight":
        # exact: speaker 123 leads 124 by 1e4 * feat[:, 9] >= 5000 on every row; clamped to 65504 both weights are equal and the
        # other 127 columns decide
        feat[:, 9] = np.abs(feat[:, 9]) + 0.5
        wl[123, 9] = 2.0e5
        wl[124, 9] = 1.9e5
    elif what == "inf_weight":
        # exact: speaker 123's logit is +Inf on every row; clamped to 65504 it ties with 124 on column 9
        feat[:, 9] = np.abs(feat[:, 9]) + 0.5
        wl[123, 9] = np.inf
        wl[124, 9] = 1.0e5
    elif what == "nan_weight":
        # exact: speaker 200's logit is NaN on every row and never wins; clamped, the NaN becomes -65504 and -65504 * feat[:, 9]
        # (feat < 0) the largest logit of every row
        feat[:, 9] = -np.abs(feat[:, 9]) - 0.5
        wl[200, 9] = np.nan
    elif what == "feature":
        # exact: 77 leads 78 by 0.1 * 2e5 - 100 * 100 = 1e4; with the feature clamped to 65504 + 65504 / 2048 speaker 78 wins by 3400
        feat[row, 3] = 2.0e5; wl[77, 3] = 1.0; wl[78, 3] = 0.9; wl[78, 4] = 100.0; feat[row, 4] = 100.0
    elif what == "feature_65519":
        # just above the threshold: 65519 against a bias of 65515 on a speaker with zero weights
        feat[row, 3] = 65519.0; wl[77, :] = 0.0; wl[77, 3] = 1.0; wl[78, :] = 0.0
        bl[78] = 65515.0; bl[77] = 0.0
    elif what == "bias":
        bl[200] = 1.0e5                                                  # the bias is added in fp32 in every form: 200 wins everywhere
    elif what == "nan_row":
        feat[row, :] = np.nan
    f, ids = _head_ids(feat, wl, bl, form)
    if form != "split":
        assert np.array_equal(np.isnan(f), np.isnan(feat)) and np.array_equal(f[~np.isnan(f)], feat[~np.isnan(feat)])
    _check_ids(f, ids, wl, bl, "%s %s" % (form, what))
    if what in ("feature", "feature_65519"):
        assert ids[row] == 77
    if what in ("weight", "inf_weight"):
        assert (ids == 123).all()
    if what == "nan_weight":
        assert not (ids == 200).any()
    if what == "bias":
        assert (ids == 200).all()
    if what == "nan_row":
        assert np.isnan(f[row]).all()                                    # the NaN is in the call's output; the other rows are checked above


# ------------------------------------------------------------------------------------------------ grouped convs and the rest, through tal_tds_fwd
class _Tracer:
    """TDS(80, [80, 800, 1120, 1440], [1, 1, 1]) with synthetic weights and ONE tracer path: input sample x[b0, 2 t0', 79] = V
    travels unchanged (one-hot first conv, zeroed conv / fc rows on its channel, residual adds) to the site under test, where a
    bias or a doubling weight lifts that one element beyond 65504.  Every activation is also computed in float64 on the host, so
    the case checks its own premise: exactly one out-of-range value at the site, none at any earlier site."""
    SITES = ["s0.down", "s0.conv", "s0.fc0", "s0.fc3", "s1.down", "s1.conv", "s1.fc0", "s1.fc3", "s2.down", "s2.conv", "s2.fc0"]
    CPG = [10, 14, 18]
    G0 = 79                       # last group: last column block of every layer

    def __init__(self):
        from tal_asrd_amd import TDS, synth
        torch.manual_seed(3)
        self.tds = TDS(80, [80, 800, 1120, 1440], [1, 1, 1])
        sd = synth.fill_state_dict({"g." + k: tuple(v.shape) for k, v in self.tds.state_dict().items()})
        self.base = {k: torch.from_numpy(sd["g." + k].copy()) for k in self.tds.state_dict()}
        self.tds.to(dev())
        self.B, self.T = 2, 2400
        self.x0 = torch.randn(self.B, self.T, 80, generator=torch.Generator().manual_seed(4))

    def ch(self, s):
        return self.G0 * self.CPG[s] + 3

    def params(self, site, lift):
        """state dict with the tracer path; `lift`: the planted value V arrives at `site` as V (lift by bias 0) ... see plant()"""
        p = {k: v.clone() for k, v in self.base.items()}
        RW = 0.5
        for s in range(3):
            c = self.ch(s)
            pre = "blocks.%d." % s
            dw, db = p[pre + "0.weight"], p[pre + "0.bias"]
            dw[c] = 0.0
            db[c] = 0.0
            if s == 0:
                dw[c, 0, 0] = 1.0                                        # y[t, c] = x[2 t, 79]
            else:
                dw[c, 3, 0] = 1.0                                        # input channel 3 of the group = the tracer of the stage before
            blk = pre + "1.0."
            p[blk + "resweight"].fill_(RW)
            p[blk + "conv.0.weight"][c] = 0.0
            p[blk + "conv.0.bias"][c] = 0.0
            p[blk + "fc.0.weight"][7] = 0.0                              # fc0 row 7: the tracer's doubling row (off unless the site is fc0)
            p[blk + "fc.0.bias"][7] = 0.0
            p[blk + "fc.3.weight"][c] = 0.0
            p[blk + "fc.3.bias"][c] = 0.0
        return p, RW

    T_OUT = [1190, 585, 283]      # frames per item after each stage at T = 2400

    def frame(self, s, pos):
        """frame of stage s the tracer sits in: the first frame of the first item, the last valid frame of the last item (a partial
        time tile at every tile length), or one in the middle"""
        return {"first": 0, "last": self.T_OUT[s] - 1, "mid": 44 >> s}[pos]

    def plant(self, site, val, pos="mid"):
        """-> (params, x): at `site` exactly one converted value equals `val` (finite: exactly; non-finite: Inf / NaN)."""
        p, RW = self.params(site, val)
        s = int(site[1])
        kind = site[3:]
        blk = "blocks.%d.1.0." % s
        c = self.ch(s)
        x = self.x0.clone()
        t_in = self.frame(s, pos) << (s + 1)     # tap 0 of each one-hot conv: stage frame f reads input frame f * 2^(s + 1)
        b0 = 0 if pos == "first" else self.B - 1
        finite = bool(np.isfinite(val))
        carried = min(val, 65000.0) if finite else 1.0
        if kind == "down":
            if s == 0:
                carried = val            # the first converting site: the sample itself
            else:
                p["blocks.%d.0.weight" % s][c, 3, 0] = 2.0 if finite else 1.0     # y = 2 * carried
                carried = val / 2.0 if finite else 1.0
                if not finite:
                    p["blocks.%d.0.bias" % s][c] = val
        elif kind == "conv":             # x1 = x + rw * relu(bias): lifts EVERY frame of the channel by the same amount
            p[blk + "conv.0.bias"][c] = (val - carried) / RW if finite else val
        elif kind == "fc0":
            p[blk + "fc.0.weight"][7, c, 0] = 2.0 if finite else 1.0
            carried = val / 2.0 if finite else 1.0
            if not finite:
                p[blk + "fc.0.bias"][7] = val
        elif kind == "fc3":
            p[blk + "fc.3.bias"][c] = (val - carried) / RW if finite else val
        if (val == float("-inf") or np.isnan(val)) and kind in ("conv", "fc0"):
            return None                  # relu(-inf) = 0; relu(NaN) = fmaxf(NaN, 0) = 0 in every kernel (include/tal_asrd.h)
        x[b0, t_in, self.G0] = carried
        return p, x

    def load(self, p):
        own = self.tds.state_dict()
        for k in own:
            own[k] = p[k]
        self.tds.load_state_dict(own)
        self.tds.to(dev())

    def activations64(self, p, x, dt=torch.float64):
        """activations at every converting site, in order, as [B, T, C] float64 arrays computed in `dt` on the host; last entry:
        the encoder output."""
        F = torch.nn.functional
        p = {k: v.to(dt) for k, v in p.items()}
        a = x.to(dt).permute(0, 2, 1)
        out = {}
        with torch.no_grad():
            for s in range(3):
                pre = "blocks.%d." % s
                a = F.conv1d(a, p[pre + "0.weight"], p[pre + "0.bias"], stride=2, groups=80)
                out["s%d.down" % s] = a
                blk = pre + "1.0."
                rw = float(p[blk + "resweight"])
                a = a + rw * torch.relu(F.conv1d(a, p[blk + "conv.0.weight"], p[blk + "conv.0.bias"], padding=10, groups=80))
                out["s%d.conv" % s] = a
                h = torch.relu(F.conv1d(a, p[blk + "fc.0.weight"], p[blk + "fc.0.bias"]))
                out["s%d.fc0" % s] = h
                a = a + rw * F.conv1d(h, p[blk + "fc.3.weight"], p[blk + "fc.3.bias"])
                out["s%d.fc3" % s] = a
        return {k: v.permute(0, 2, 1).double().numpy() for k, v in out.items()}

    def run_flag(self, x):
        """tal_tds_fwd through the driver with the status word read here (the fallback counter is not touched)"""
        from tal_asrd_amd import ops
        desc = self.tds._descriptor()
        y, chk = ops.tds_forward(desc, x.to(dev()), 1440, defer=True)
        torch.cuda.synchronize()
        flag = int(chk.ws[chk.off:chk.off + 4].view(torch.int32)[0])
        return y.cpu().double().numpy(), flag


@pytest.fixture(scope="module")
def tracer():
    return _Tracer()


def _window_max(a, radius):
    """running maximum over the frame axis of a [B, T] array"""
    pad = np.pad(a, ((0, 0), (radius, radius)), mode="edge")
    return np.max(np.stack([pad[:, i:i + a.shape[1]] for i in range(2 * radius + 1)]), axis=0)


def _encoder_bound(tracer, p, x, want):
    """Element-wise bound of the encoder output against float64: 4 * e32 + 11 * 2^-22 * scale, both per output frame over the
    frames its receptive field mixes (+-24 output frames).  e32 = error of the same stack computed in float32 on the host;
    the second term is the split form of the 11 stored activations in front of the output (22 mantissa bits each, layer gains
    <= 1: weights ~ 1 / sqrt(K), residual weight 0.5).  The tracer's own 6e4 raises the scale around its frame only."""
    y32 = tracer.activations64(p, x, torch.float32)["s2.fc3"]
    e32 = _window_max(np.abs(y32 - want).max(axis=2), 24)
    scale = _window_max(np.abs(want).max(axis=2), 24)
    return (4 * e32 + 11 * 2.0 ** -22 * scale)[:, :, None]


# kernel-selection options of a flow -> the sites it is run on -> (value, position) cases beyond the full table at "mid"
FLOWS = {
    # every activation of a stage in the split form; short inputs: 64-step conv tiles, 64 x 80 dense tiles
    "split": ({}, _Tracer.SITES, [(v, pos) for pos in ("first", "last") for v in (65504.0, 65519.0, 1.0e5)]),
    # the same with the long conv tiles (256 / 128 steps): the other tile length of the matrix-core conv epilogues
    "split_long_tiles": ({"gconv_short_below": 0}, ["s0.conv", "s1.down", "s1.conv", "s2.down", "s2.conv"], None),
    # fp32 activations between the kernels: the value is converted by its CONSUMER -- the block conv's slab fill from fp32 input
    # (after a resize conv), the guarded split pass (after a block conv), the next resize conv's slab fill (after fc3)
    "fp32_activations": ({"tds_fp32_activations": 1}, _Tracer.SITES, None),
    # first resize conv computed inside the first block conv's launch
    "c1_fused": ({"gconv_c1_fuse": 1}, ["s0.down", "s0.conv"], [(v, pos) for pos in ("first", "last") for v in (65504.0, 65519.0)]),
}
# (1e5 matters beside 65519: its unclamped halves are Inf / -Inf and decode to NaN downstream, which no later site's maximum
#  sees -- a site that lost its note_range is then not covered up by the next one)
SHORT_CASES = [(65504.0, "mid"), (65519.0, "mid"), (1.0e5, "mid"), (float("nan"), "mid"), (65519.0, "first"), (65519.0, "last"),
               (1.0e5, "first"), (1.0e5, "last")]


@pytest.mark.parametrize("flow,site", [(f, s) for f in FLOWS for s in FLOWS[f][1]])
def test_tds_sites(tracer, flow, site):
    """Every converting site of an encoder call in turn (first resize conv, block convs at 10 / 14 / 18 channels per group, both
    dense layers of a block, the matrix-core resize convs), in the all-split flow at both conv tile lengths, in the
    fp32-activation flow (slab fill from fp32 input, guarded split pass) and with the fused first conv: the value planted at
    that site alone -- first frame of item 0, last valid frame of item B - 1, mid-sequence; last column block -- raises
    tal_tds_fwd's status word when it is beyond 65504 or not finite and leaves it clear at 65504 and 6e4, where the whole
    output matches float64 element-wise (_encoder_bound).  The flow each call takes is asserted from tal_tds_out_split."""
    from tal_asrd_amd import _native as N_
    import ctypes as C
    opts, _, extra = FLOWS[flow]
    cases = [(v, "mid") for v, _ in TOP] + extra if extra is not None else SHORT_CASES
    must_of = dict((repr(v), m) for v, m in TOP)
    order = _Tracer.SITES
    saved = {k: N_.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            N_.set_option(k, v)
        for val, pos in cases:
            must = must_of[repr(val)]
            planted = tracer.plant(site, val, pos)
            if planted is None:
                continue
            p, x = planted
            act = tracer.activations64(p, x)
            # premise, checked in float64: one out-of-range value at the site, none before it
            for name in order[:order.index(site)]:
                assert not R.out_of_range(act[name].astype(np.float32)).any(), ("premise: earlier site out of range", site, name, val)
            n_out = int(R.out_of_range(act[site].astype(np.float32)).sum())
            if site.endswith("conv") and np.isfinite(val) and must:
                assert n_out == 1, ("premise", site, val, n_out)
            else:
                assert (n_out >= 1) == must, ("premise", site, val, n_out)
            tracer.load(p)
            # the flow: every stage all-split (or none, with fp32 activations), as tal_tds_out_split predicts for the stack cut there
            lib = N_.lib()
            for last in (1, 2, 3):
                asked = N_.TdsDesc.from_buffer_copy(tracer.tds._descriptor(0, last))
                asked.flags |= N_.TAL_TDS_OUT_SPLIT
                assert lib.tal_tds_out_split(C.byref(asked), tracer.B, tracer.T) == (0 if flow == "fp32_activations" else 1), (flow, last)
            y, flag = tracer.run_flag(x)
            what = (flow, site, val, pos)
            if np.isnan(val):
                # clamped sites raise the word; unclamped halves carry the NaN on into the encoder output
                assert flag != 0 or not np.isfinite(y).all(), ("finite output under a clear flag", what)
                continue
            assert (flag != 0) == must, (what, flag)
            if not must:
                want = act["s2.fc3"]
                err, tol = np.abs(y - want), _encoder_bound(tracer, p, x, want)
                print("tds %s %s %g %s: max err / bound %.3f" % (flow, site, val, pos, float((err / tol).max())))
                assert bool((err <= tol).all()), (what, float((err / tol).max()))
    finally:
        for k, v in saved.items():
            N_.set_option(k, v)


@pytest.mark.range_fallback
def test_tds_fallback_from_a_late_site(tracer):
    """Through TDS.forward_time_major: a value that leaves the range only at the LAST stage's block conv makes the call re-run
    once on the exact kernels (ops.range_fallbacks + 1) and the result matches float64; the same path at 65504 does not."""
    from tal_asrd_amd import ops
    for val, must in ((65504.0, False), (65519.0, True), (7.0e4, True)):
        p, x = tracer.plant("s2.conv", val)
        tracer.load(p)
        before = ops.range_fallbacks
        y = tracer.tds.forward_time_major(x.to(dev()))
        torch.cuda.synchronize()
        assert ops.range_fallbacks == before + (1 if must else 0), (val, ops.range_fallbacks - before)
        want = tracer.activations64(p, x)["s2.fc3"]
        err = np.abs(y.cpu().double().numpy() - want)
        assert bool((err <= _encoder_bound(tracer, p, x, want)).all()), (val, float(err.max()))
