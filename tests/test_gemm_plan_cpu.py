"""csrc/gemm_plan.h on the host (plain C++): what launch_gemm launches for a dense layer.  tests/_gemm_plan_harness.cpp walks TDS
layers, exact fp32 layers, the decoder's short problems, every dense-layer option, alignments, pitches and scratch sizes at 64, 256
and 304 CUs and checks per plan: the steps' rows tile [0, M) in order, their work adds up to 2 M N K nbatch, grid = whole tiles +
tail_tiles * split K slices with tile_base + tail_tiles = all tiles, split is 0 or 2..8 with >= 4 K steps per slice, the slices fit
the scratch, grids stay below 2^31, umulhi(t, magic) == t / tiles_n (and tiles_m) around every multiple, at most
GEMM_PLAN_MAX_STEPS steps.  Every arm of the dispatcher must be reached, and every launch must equal the one the if-chain dispatcher
made before the plan existed: tests/gemm_plan_parent.txt is that dispatcher's record for the same sweep (one line per launch: kernel
and template arguments, grid, block, M, row offset, tiles_n, tiles_m, n_major, tile_base, split, tail_tiles, stagger).  No GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_plan_invariants_arms_and_parent_decisions(tmp_path):
    exe = str(tmp_path / "gemm_plan_harness")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(HERE, "_gemm_plan_harness.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    out = p.stdout.splitlines()
    assert p.returncode == 0, "\n".join(out[-3:]) + p.stderr
    arms = {w[1]: int(w[2]) for w in (line.split() for line in out) if w[0] == "A"}
    assert len(arms) == 31 and all(n > 0 for n in arms.values()), arms
    with open(os.path.join(HERE, "gemm_plan_parent.txt")) as f:
        parent = f.read().splitlines()
    case, k = None, 0
    for line in out:
        if line.startswith("C "):
            case = line
        elif line.startswith("L "):
            assert k < len(parent) and line[2:] == parent[k], "launch %d: %r, before the plan %r (%s)" % (
                k, line[2:], parent[k] if k < len(parent) else None, case)
            k += 1
    assert k == len(parent)
