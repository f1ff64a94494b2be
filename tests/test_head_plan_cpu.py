"""csrc/head_plan.h on the host (the header is plain C++ there): the run partition the streaming heads (csrc/head_stream.h,
csrc/soft_embed.hip) share.  tests/_head_plan_harness.cpp walks tile widths 128 / 64, one / two workgroups per CU at 256 CUs, ten
row counts, thirteen head widths and nine grid overrides and checks per combination: grid >= 1, hp <= 16 (the merge kernels take
one partial per lane), no row block meets more workgroups than hp, and the runs tile [0, U) with block_of as their inverse.  No GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_slot_bound_and_run_partition(tmp_path):
    exe = str(tmp_path / "head_plan_harness")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(HERE, "_head_plan_harness.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    words = p.stdout.split()
    assert words[0] == "combinations" and int(words[1]) == 2 * 2 * 10 * 13 * 9, p.stdout
    # the bound is tight: some shape of the table needs all 16 slots, so a plan that allowed 17 would show here
    assert words[2] == "worst_hp" and int(words[3]) == 16, p.stdout
