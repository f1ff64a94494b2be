"""The fp16x3 dense layers' exact integer model and the case tables of the short-input kernel (gemm_s64_kernel, csrc/gemm_s64.hip)
and of gemm_plan's row split, for tests/test_dense_forms_cpu.py (no GPU) and tests/test_gpu_dense_mfma_shape.py (GPU).  numpy only.

1. The model.  Operands in the split format with small integer halves: every partial sum of a kernel is exact in fp32 whatever
   the summation order, so the expected output holds BIT FOR BIT.
2. short_cases(cus) / row_split_cases(cus): shapes and options, each with the form it is there for.
3. expect_plan(case, cus): a restatement of the part of gemm_plan (csrc/gemm_plan.h) these cases rest on -- the 64 x 80 arm, the
   256 x 160 arm with its row split, and "neither, and no K slices: whole 128 x 160 tiles".  tests/test_dense_forms_cpu.py holds it
   to the header at 64, 256 and 304 CUs.  It is not the whole planner: it raises where a case leaves what it restates.
"""
import numpy as np


def cdiv(a, b):
    return -(-a // b)


# ---- the integer model ---------------------------------------------------------------------------------------------------------------
def pack(hi, lo):
    """the fp16x3 operand format (include/tal_asrd.h): per row and 32-wide K block, 32 hi halves then 32 lo halves"""
    rows, K = hi.shape
    out = np.empty((rows, K // 32, 64), dtype=np.float16)
    out[:, :, :32] = hi.reshape(rows, K // 32, 32)
    out[:, :, 32:] = lo.reshape(rows, K // 32, 32)
    return out


def unpack(p):
    """the values of a packed array [rows, blocks, 64], float64: hi + lo / 2^11"""
    p = p.astype(np.float64)
    return (p[:, :, :32] + p[:, :, 32:] / 2048.0).reshape(p.shape[0], -1)


def host_split(y):
    """host split of exact fp32 values inside the fp16 range: hi = fp16(y), lo = fp16((y - hi) * 2^11)"""
    hi = y.astype(np.float16)
    lo = ((y - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return pack(hi, lo)


def int_operand(rng, rows, K):
    hi = rng.integers(-2, 3, size=(rows, K)).astype(np.float32)
    lo = rng.integers(-8, 9, size=(rows, K)).astype(np.float32)
    return hi, lo


def exact_model(M, N, K):
    """operands with integer halves and the exact results of both layers.  Model: pre = sum hi.hi' + b + 2^-11 sum (hi.lo' + lo.hi')
    (lo.lo' is dropped by the kernels by design); mode 1: max(pre, 0); mode 2: res + 0.5 pre with res = rh + 2^-11 rl.  Every term
    is an integer: the float64 products below are exact in any order, and 4 K + 4 < 4096 keeps every fp32 partial sum of a kernel
    exact too.  Returns the halves, the bias, the residual as a plain fp32 matrix (exact), pre (float64) and exp[mode] (fp32)."""
    assert 4 * K + 4 < 4096
    rng = np.random.default_rng(1000 * N + K)
    xh, xl = int_operand(rng, M, K)
    wh, wl = int_operand(rng, N, K)
    b = rng.integers(-4, 5, size=N).astype(np.float32)
    rh, rl = int_operand(rng, M, N)          # the split residual of the mode-2 layer
    d = lambda a: a.astype(np.float64)
    hh = d(xh) @ d(wh).T
    xx = d(xh) @ d(wl).T + d(xl) @ d(wh).T
    pre = hh + d(b) + xx / 2048.0
    assert float(np.abs(pre).max()) < 4 * K + 8
    res = d(rh) + d(rl) / 2048.0
    rf = res.astype(np.float32)
    assert np.array_equal(d(rf), res)
    exp = {}
    for mode, y in ((1, np.maximum(pre, 0.0)), (2, res + 0.5 * pre)):
        y32 = y.astype(np.float32)
        assert np.array_equal(d(y32), y)                          # the model's values ARE fp32 values
        exp[mode] = y32
    return dict(xh=xh, xl=xl, wh=wh, wl=wl, b=b, rh=rh, rl=rl, rf=rf, pre=pre, exp=exp)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
OPTION_DEFAULTS = {"gemm_s64_below": 2, "gemm_s64_rows": 0, "gemm_s64_order": 0}

# run kinds of the GPU test as (mode, split output, guarded call, residual form)
S64_RUNS = [(1, 0, False, None), (2, 0, False, "f32"), (1, 1, False, None), (1, 1, True, None), (2, 1, True, "split"), (2, 0, True, "split"),
            (2, 1, True, "f32")]
F32_RUNS = S64_RUNS[:2]                     # N % 160 != 0: fp32 in and out only
ROW_SPLIT_RUNS = [(1, 0, False, None), (1, 1, True, None), (2, 1, True, "split")]


def runs_of(case):
    if case["group"].startswith("row_split"):
        return ROW_SPLIT_RUNS
    return S64_RUNS if case["N"] % 160 == 0 else F32_RUNS


def _case(group, M, N, K, options=None, **form):
    opts = dict(options or {})
    name = "%s-%dx%dx%d" % (group, M, N, K) + "".join("-%s%d" % (k.replace("gemm_s64_", ""), v) for k, v in sorted(opts.items()))
    return dict(name=name, group=group, M=M, N=N, K=K, options=opts, form=form)


def short_case_names():
    """the ids of short_cases at any CU count (one shape depends on the CU count: its id does not name it)"""
    return [c["id"] for c in short_cases(256)]


def short_cases(cus):
    """the cases that gemm_s64_kernel must take as ONE launch.  form: the fields of the launch the case is there for."""
    cases = []
    # K-loop remainders (K / 32 mod 4 = 0 .. 3) and the short prologue (K / 32 < 4: dropped loads), both tile heights
    for K in range(32, 289, 32):
        cases.append(_case("k_rem", 129, 160, K, {"gemm_s64_rows": 2}, bm=32, tiles_m=5, tiles_n=2))
        cases.append(_case("k_rem", 129, 160, K, {"gemm_s64_rows": 1}, bm=64, tiles_m=3, tiles_n=2))
    # the tile walk: grids of every residue mod 8, tiles_n == 1 (no magic division), one valid row in the last tile
    for i in range(8):
        cases.append(_case("walk32", 129 + 32 * i, 80, 64, bm=32, grid=5 + i, tiles_n=1, n_major=0))
    for i in range(8):
        cases.append(_case("walk64", 129 + 64 * i, 80, 64, {"gemm_s64_rows": 1}, bm=64, grid=3 + i, tiles_n=1, n_major=0))
    # both tile orders where they put different tiles into a workgroup: 63-row tail, whole tiles, tiles_n = 10
    for M, N, K in ((191, 160, 96), (192, 320, 128), (200, 800, 64)):
        for order in (0, 1, 2):
            cases.append(_case("order", M, N, K, {"gemm_s64_order": order} if order else {},
                               n_major=int(M < N) if order == 0 else order - 1, tiles_n=N // 80))
    # (191 rows are a last tile of 31 rows on 32-row tiles, which the plan takes here: the same shape on 64-row tiles, 63 valid rows)
    cases.append(_case("tail63", 191, 160, 96, {"gemm_s64_rows": 1}, bm=64, tiles_m=3, tiles_n=2))
    # 64-row tiles chosen by the plan itself: 32-row tiles would be more than one per CU
    cases.append(_case("plan64", 32 * (cus // 2) + 8 + 96, 160, 64, bm=64))
    # N no multiple of 160
    cases.append(_case("n240", 300, 240, 160, tiles_n=3))
    for c in cases:
        c["id"] = c["name"] if c["group"] != "plan64" else "plan64"
    return cases


def check_short_form(case, cus):
    """the case runs as one launch of gemm_s64_kernel in the form it is there for; says which field is off otherwise"""
    steps = expect_plan(case, cus)
    assert len(steps) == 1 and steps[0][0] == "s64", "%s at %d CUs is no single 64 x 80 launch: %r" % (case["name"], cus, steps)
    _, rows, row0, bm, n_major, tiles_m, tiles_n, grid = steps[0]
    got = dict(rows=rows, row0=row0, bm=bm, n_major=n_major, tiles_m=tiles_m, tiles_n=tiles_n, grid=grid)
    for k, v in case["form"].items():
        assert got[k] == v, "%s at %d CUs: %s is %r, the case needs %r" % (case["name"], cus, k, got[k], v)
    return steps


def row_split_cases(cus):
    """one round of 256 x 160 tiles and a second launch for the remaining rows, by the kind of the second launch.  The remainders
    are 129 / 3000 / 4000 rows at 256 CUs and shrink with the CU count where they would leave their arm (a device with a quarter of
    the CUs takes a remainder of 3000 x 320 on 128 x 160 tiles, not on 64 x 80)."""
    r64 = min(3000, 24 * cus)                # 64-row tiles: more 32-row tiles than CUs, at most two 64-row tiles per CU
    r128 = min(4000, 16 * cus - 96)          # too many 64 x 80 tiles (> 2 per CU), fewer than a round of 256-row tiles
    cases = [
        dict(id="row_split_s64_32", M=256 * cus + 129, N=160, K=64, second=("s64", 32)),
        dict(id="row_split_s64_64", M=256 * (cus // 2) + r64, N=320, K=64, second=("s64", 64)),
        dict(id="row_split_glds160", M=256 * (cus // 5) + r128, N=800, K=64, second=("glds160", 128)),
    ]
    for c in cases:
        c.update(group="row_split", options={}, name="%s-%dx%dx%d" % (c["id"], c["M"], c["N"], c["K"]))
        M, N = c["M"], c["N"]
        tiles_n = cdiv(N, 160)
        nb, rows1 = cdiv(M, 256) * tiles_n, (cus // tiles_n) * 256
        what = "%s at %d CUs: " % (c["name"], cus)
        assert nb >= cus, what + "nb = %d 256-row tiles are less than one round (nb >= cus)" % nb
        assert nb < 2 * cus, what + "nb = %d tiles are two rounds or more (nb < 2 cus)" % nb
        assert nb % cus != 0, what + "nb = %d tiles are whole rounds (nb %% cus != 0)" % nb
        assert 128 < M - rows1 <= 4096, what + "%d rows remain behind the round (128 < M - rows1 <= 4096)" % (M - rows1)
        steps = expect_plan(c, cus)
        assert len(steps) == 2 and steps[0][:3] == ("w64", rows1, 0) and steps[1][1:3] == (M - rows1, rows1), what + "steps %r" % (steps,)
        kind, bm = c["second"]
        assert steps[1][0] == kind and (kind != "s64" or steps[1][3] == bm), what + "the second launch is %r, the case needs %s with %d-row tiles" % (
            steps[1], kind, bm)
    return cases


def row_split_case_names():
    return [c["id"] for c in row_split_cases(256)]


def expect_plan(case, cus):
    """the launches of a case in order.  64 x 80: ("s64", rows, row0, bm, n_major, tiles_m, tiles_n, grid); 256 x 160 and 128 x 160:
    ("w64" | "glds160", rows, row0, grid, split).  Packed, 16-byte aligned operands in the fp16x3 form, modes 1 / 2, K % 32 == 0."""
    M, N, K = case["M"], case["N"], case["K"]
    o = dict(OPTION_DEFAULTS)
    o.update(case.get("options", {}))
    assert set(o) == set(OPTION_DEFAULTS), "an option that expect_plan does not restate: %r" % (o,)
    assert M > 128 and K % 32 == 0
    steps, row0 = [], 0
    while True:
        # short inputs: whole 64 x 80 tiles while they fit one round of gemm_s64_below workgroups per CU
        if N % 80 == 0 and cdiv(M, 64) * (N // 80) <= o["gemm_s64_below"] * cus:
            tiles_n = N // 80
            half = o["gemm_s64_rows"] == 2 or (o["gemm_s64_rows"] == 0 and cdiv(M, 32) * tiles_n <= cus)
            bm = 32 if half else 64
            tiles_m = cdiv(M, bm)
            n_major = {1: 0, 2: 1}.get(o["gemm_s64_order"], int(M < N))
            steps.append(("s64", M, row0, bm, n_major, tiles_m, tiles_n, tiles_m * tiles_n))
            return steps
        # every other launch of these cases: a K slice has at least four K steps and a tile at least two slices; the 128 x 96 tiles need N % 96 == 0
        assert K // 32 < 8 and N % 96 != 0, "expect_plan restates launches without K slices and 96-wide tiles only"
        tiles_n = cdiv(N, 160)
        nb = cdiv(M, 256) * tiles_n
        if nb >= cus:
            # one full round and a remainder of a few thousand rows: the round's row blocks are a launch of their own
            rb = cus // tiles_n
            rows1 = rb * 256
            if nb < 2 * cus and nb % cus != 0 and rb >= 1 and 128 < M - rows1 <= 4096 and len(steps) < 2:
                steps.append(("w64", rows1, row0, rb * tiles_n, 0))
                row0 += rows1
                M -= rows1
                continue
            steps.append(("w64", M, row0, nb, 0))
            return steps
        steps.append(("glds160", M, row0, cdiv(M, 128) * tiles_n, 0))
        return steps
