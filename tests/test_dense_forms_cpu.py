"""tests/_dense_forms.py on the host: the case tables of the short-input kernel and of the row split, their restated plan
(expect_plan) against csrc/gemm_plan.h itself -- tests/_gemm_plan_query.cpp, compiled here with g++ like the harness of
tests/test_gemm_plan_cpu.py -- at 64, 256 and 304 CUs, and the exact integer model that tests/test_gpu_dense_mfma_shape.py compares
the kernels with.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from tests import _dense_forms as F

HERE = os.path.dirname(os.path.abspath(__file__))
CU_COUNTS = (64, 256, 304)
WS = 1024 * 128 * 160 * 4                   # gemm_splitk_ws_bytes(), as in tests/_gemm_plan_harness.cpp
OPTION_ORDER = ["gemm_s64_below", "gemm_no_w64", "gemm_no_glds", "gemm_no_splitk4", "gemm_no_splitk_tail", "gemm_no_row_split", "gemm_no_n96",
                "gemm_global_loads", "gemm_s64_rows", "gemm_s64_order", "gemm_w64_stagger"]


def _calls():
    """(cus, case, run kind) of every case of both tables in the run kinds of the GPU test"""
    for cus in CU_COUNTS:
        for case in F.short_cases(cus) + F.row_split_cases(cus):
            for run in F.runs_of(case):
                yield cus, case, run


def _line(cus, case, run):
    mode, out_split, guarded, res = run
    M, N, K = case["M"], case["N"], case["K"]
    # the scratch the GPU test passes: tal_linear_workspace_bytes (gemm_wants_scratch), at least 16 bytes
    ws = WS if M > 512 and K >= 256 else 16
    o = dict(F.OPTION_DEFAULTS)
    o.update(case["options"])
    return " ".join(str(v) for v in [cus, M, N, K, mode, out_split, int(res == "split"), int(guarded), ws] + [o.get(k, 0) for k in OPTION_ORDER])


def _header_plans(tmp_path, lines):
    exe = str(tmp_path / "gemm_plan_query")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(HERE, "_gemm_plan_query.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    plans, steps = [], []
    for w in (line.split() for line in p.stdout.splitlines()):
        if w[0] == "S":
            kernel = w[1]
            rows, row0, bm, bn, waves, n_major, tiles_m, tiles_n, grid, split = (int(x) for x in w[2:])
            if kernel == "s64":
                assert bn == 80 and waves * 16 == bm and split == 0
                steps.append(("s64", rows, row0, bm, n_major, tiles_m, tiles_n, grid))
            else:
                assert kernel in ("w64", "glds160"), w
                assert (bm, bn) == ((256, 160) if kernel == "w64" else (128, 160))
                steps.append((kernel, rows, row0, grid, split))
        else:
            assert w[0] == "E" and int(w[1]) == len(steps), w
            plans.append(steps)
            steps = []
    assert len(plans) == len(lines)
    return plans


def test_expect_plan_equals_the_header(tmp_path):
    calls = list(_calls())
    plans = _header_plans(tmp_path, [_line(*c) for c in calls])
    for (cus, case, run), plan in zip(calls, plans):
        assert F.expect_plan(case, cus) == plan, (case["name"], cus, run)


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_cases_take_the_forms_they_are_there_for(cus):
    cases = F.short_cases(cus)
    assert [c["id"] for c in cases] == F.short_case_names() and len(set(F.short_case_names())) == len(cases)
    for case in cases:
        (step,) = F.check_short_form(case, cus)
        assert step[1:3] == (case["M"], 0) and step[7] == step[5] * step[6]
    # K / 32 = 1 .. 9 in both tile heights: every remainder of the K loop (four steps per pass), without and behind a pass, and
    # the prologue with fewer than four tiles
    for rows, bm in ((2, 32), (1, 64)):
        ks = [c["K"] // 32 for c in cases if c["group"] == "k_rem" and c["options"]["gemm_s64_rows"] == rows and c["form"]["bm"] == bm]
        assert ks == list(range(1, 10))
    # the tile walk deals a grid to the 8 XCDs by grid >> 3 and grid & 7: every residue, both tile heights
    for group in ("walk32", "walk64"):
        grids = [F.expect_plan(c, cus)[0][7] for c in cases if c["group"] == group]
        assert sorted(g % 8 for g in grids) == list(range(8)), (group, grids)
    # last tiles with one valid row and with all but one, in both heights
    tails = {(F.expect_plan(c, cus)[0][3], c["M"] % F.expect_plan(c, cus)[0][3]) for c in cases}
    assert {(32, 1), (64, 1), (32, 31), (64, 63)} <= tails, tails
    # both orders at every "order" shape, and tiles_n = 10 through the magic division
    orders = {(c["M"], F.expect_plan(c, cus)[0][4]) for c in cases if c["group"] == "order"}
    assert orders == {(M, n) for M in (191, 192, 200) for n in (0, 1)}


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_row_split_cases_split(cus):
    cases = F.row_split_cases(cus)              # (asserts the plan's conditions, with the condition in the message)
    assert [c["id"] for c in cases] == F.row_split_case_names()
    for case in cases:
        first, second = F.expect_plan(case, cus)
        assert first[1] % 256 == 0 and second[2] == first[1] and first[1] + second[1] == case["M"]


def test_exact_model_of_every_case():
    """the expected values are fp32 values (asserted by the model), their split form decodes back to them exactly, and |pre| < 4 K + 8"""
    seen = set()
    for case in F.short_cases(256) + F.row_split_cases(256):
        key = (case["M"], case["N"], case["K"])
        if key in seen:
            continue
        seen.add(key)
        M, N, K = key
        m = F.exact_model(M, N, K)
        assert float(np.abs(m["pre"]).max()) < 4 * K + 8
        if N % 32 != 0:                          # (fp32 in and out only: no split form of an [M, N] matrix)
            continue
        assert np.array_equal(m["rf"].astype(np.float64), F.unpack(F.pack(m["rh"], m["rl"])))
        for mode in (1, 2):
            y = m["exp"][mode]
            assert y.dtype == np.float32 and float(np.abs(y).max()) < 65504.0
            assert np.array_equal(F.unpack(F.host_split(y)), y.astype(np.float64)), (key, mode)
