"""csrc/gconv_plan.h on the host (plain C++): what the grouped-conv entry points launch.  tests/_gconv_plan_harness.cpp walks the
seven entries (tal_gconv_s2 / res, their fp16x3 and any-k forms, the fused resize + block conv) over the stock widths, other group
counts and odd widths, T = 1..300 and 30-second to 1-hour lengths, B = 1..64, every option, misaligned x, every split form, the
folded mean, kernel sizes 1..63, the 2 GiB bound and a grid past 2^31 blocks, at 64, 256 and 304 CUs, and checks per plan: the
tiles cover T_out and one fewer does not, whole group blocks, the 1-D grid has n_tt, n_gb > 0 and fewer than 2^31 blocks and the 3-D
grid has both 0, LDS bytes equal the kernel's own formula and stay within 160 KB, a matrix-core plan fits the 2 GiB bound, split
input needs C_in % 32 == 0 and (CIG x GB) % 4 == 0, split output C_out % 32 == 0, work = 2 B T_out C_out cig ks, short tiles exactly
when the long ones give fewer than short_below x cus workgroups; per layout: 32 nk >= (ntap - 1) pitch + nch, pitch >= nch, perm_nk
a multiple of 4 within nk(0), the weight table as large as the packer's element count, the shift-18 table exactly for 18 / 18 /
stride 1.  Every arm must be reached, and every launch, every refusal (with its message) and every answer of the 1 -> 10 predicate
must equal what the dispatchers made of the same call before the plan existed.  Their output for the same sweep has one line per
launch (kernel and template arguments, grid, block, LDS bytes, n_tt, n_gb, nb_total, T_out; per first resize conv also "split=
fold=", the old gconv_s2_can_split / gconv_s2_can_fold_mean); tests/gconv_plan_parent.txt keeps it as record() folds it: per kernel
instantiation, grid form, block and LDS bytes (or per refusal text) one line with the number of calls that got it and the sha256 of
those calls and their lines in sweep order.  A changed rule shows as calls that moved from one line to another.  No GPU."""
import collections
import hashlib
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def record(lines):
    """The harness's (or the old dispatchers') "C" / "L" / "P" lines -> the lines of tests/gconv_plan_parent.txt."""
    groups, case = collections.defaultdict(list), None
    for line in lines:
        if line.startswith("C "):
            case = line
        elif line.startswith(("L ", "P ")):
            w = line[2:].split()
            if line.startswith("L ") and w[0] not in ("refused:", "none"):       # kernel<template>(arguments) grid block LDS n_tt,n_gb,nb_total T_out
                what = "%s grid=%s block=%s lds=%s" % (w[0].split("(")[0], "x,y,z" if w[4].startswith("0,") else "1-D", w[2], w[3])
            else:       # a refusal's text, "none", or the predicates' answers
                what = line[2:]
            groups[what].append(case + "\n" + line + "\n")
    return ["%5d %s %s" % (len(g), hashlib.sha256("".join(g).encode()).hexdigest()[:16], what) for what, g in sorted(groups.items())]


def test_plan_invariants_arms_and_parent_decisions(tmp_path):
    exe = str(tmp_path / "gconv_plan_harness")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(HERE, "_gconv_plan_harness.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    out = p.stdout.splitlines()
    assert p.returncode == 0, "\n".join(out[-3:]) + p.stderr
    arms = {w[1]: int(w[2]) for w in (line.split() for line in out) if w[0] == "A"}
    assert len(arms) == 56 and all(n > 0 for n in arms.values()), arms
    with open(os.path.join(HERE, "gconv_plan_parent.txt")) as f:
        parent = f.read().splitlines()
    moved = sorted(set(record(out)) ^ set(parent), key=lambda line: line[23:])
    assert not moved, "calls, digest, launch -- now or before the plan, not both:\n" + "\n".join(moved)
