"""csrc/turns_plan.h on the host (the header is plain C++ there): tile counts, the workspace offsets of tal_speaker_turns_fwd and
tal_segment_mean_fwd, the chunk count of a range and the bound on the chunks of a call.  tests/_turns_plan_harness.cpp is a
stand-alone program with its own main; it is built with -fsanitize=address,undefined and writes every region of every layout into a
buffer of exactly the planned size, so an overlap, an overrun or a signed overflow in the arithmetic stops it.  No GPU, and nothing
under a sanitizer is loaded into Python."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_layouts_and_chunk_bound_under_sanitizers(tmp_path):
    exe = str(tmp_path / "turns_plan_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "_turns_plan_harness.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    words = p.stdout.split()
    assert words[0] == "combinations" and int(words[1]) == 14 + 5 * 11 + 8 * 8 * 6, p.stdout
