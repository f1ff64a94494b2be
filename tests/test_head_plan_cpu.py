"""csrc/head_plan.h on the host (the header is plain C++ there): the run partition the streaming heads (csrc/head_stream.h,
csrc/soft_embed.hip) share.  tests/_head_plan_harness.cpp walks tile widths 128 / 64, one / two workgroups per CU at 256 CUs, ten
row counts, thirteen head widths and nine grid overrides and checks per combination: grid >= 1, hp <= 16 (the merge kernels take
one partial per lane), no row block meets more workgroups than hp, and the runs tile [0, U) with block_of as their inverse.

With the argument "calls" the harness plans every call of the sweep in tests/_head_call_sweep.h -- the six entries (the LM ones with
and without a projection, tal_soft_embed_fwd with values of its own and with values = w) and their queries over 0 .. 44,983 rows
around every threshold, head widths 1 .. 40,000, five (E, D) pairs, k = 1 .. 16, every form and grid option, 64 / 256 / 304 CUs, row
pitches E, E + 4 and E + 2, each operand and the workspace off the 16-byte grid, workspaces of exactly the needed bytes, one byte
less, one and ten rows' worth, none and ample -- and checks per plan: the partial arrays one behind the other, as long as the
kernels' indexing makes them, ending at `need` and aligned for the accesses made to them; hp <= 16 and no row block meeting more
workgroups; the form exactly by the rule (shape, alignment, option, threshold); the generic chunk at least one row, covering M, its
logits inside the workspace; need (+ the projected rows) <= the query's answer; nothing named by a refused plan.  Every arm must be
reached, and every refusal (with its message), every launch (kernel instantiation, grid, arguments: sizes, pitches, addresses inside
the workspace, row chunks) and every query's answer must equal what the entry points made of the same call before the plan existed.
Their output for the same sweep -- the host halves of the three files as they were, on stub kernels that write the harness's lines
-- is kept in tests/head_call_parent.txt as record() folds it: per entry and refusal text (numbers as #) or sequence of kernel
instantiations one line with the number of calls that got it and the sha256 of those calls, their lines and their queries' answers
in sweep order.  A changed rule shows as calls that moved from one line to another.  The harness's launch lines are its own model
of the few lines an entry point puts around the plan (which offset goes to which kernel argument, launch_linear or launch_linear_ld,
the rows-only path): this test pins the header; that the .hip files use the plan's fields as modelled is what the GPU tests of the
three heads check.  No GPU."""
import collections
import hashlib
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def build(tmp_path):
    exe = str(tmp_path / "head_plan_harness")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(HERE, "_head_plan_harness.cpp"), "-o", exe], check=True)
    return exe


def test_slot_bound_and_run_partition(tmp_path):
    p = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    words = p.stdout.split()
    assert words[0] == "combinations" and int(words[1]) == 2 * 2 * 10 * 13 * 9, p.stdout
    # the bound is tight: some shape of the table needs all 16 slots, so a plan that allowed 17 would show here
    assert words[2] == "worst_hp" and int(words[3]) == 16, p.stdout


def record(lines):
    """The harness's (or the old entry points') "C" / "L" / "Q" lines -> the lines of tests/head_call_parent.txt."""
    groups, case, what = collections.defaultdict(list), None, None
    for line in lines:
        if line.startswith("C "):
            case, entry = line, line.split()[1]
        elif line.startswith("L "):
            if line.startswith("L refused"):
                what = entry + " " + re.sub(r"\d+", "#", line[2:])
            elif line == "L none":
                what = entry + " none"
            else:       # the launches: name<template arguments>[grid](arguments) ... n=<launches> last=<launch>
                names = [re.split(r"[\[(]", w)[0] for w in line[2:].split() if not w.startswith(("n=", "last="))]
                what = entry + " " + " ".join(dict.fromkeys(names))
            case += "\n" + line
        elif line.startswith("Q "):
            groups[what].append(case + "\n" + line + "\n")
    return ["%5d %s %s" % (len(g), hashlib.sha256("".join(g).encode()).hexdigest()[:16], what) for what, g in sorted(groups.items())]


def test_call_plan_invariants_arms_and_parent_decisions(tmp_path):
    p = subprocess.run([build(tmp_path), "calls"], capture_output=True, text=True)
    out = p.stdout.splitlines()
    assert p.returncode == 0, "\n".join(out[-3:]) + p.stderr
    arms = {w[1]: int(w[2]) for w in (line.split() for line in out) if w[0] == "A"}
    assert len(arms) == 52 and all(n > 0 for n in arms.values()), arms
    with open(os.path.join(HERE, "head_call_parent.txt")) as f:
        parent = f.read().splitlines()
    moved = sorted(set(record(out)) ^ set(parent), key=lambda line: line[23:])
    assert not moved, "calls, digest, entry and outcome -- now or before the plan, not both:\n" + "\n".join(moved)
