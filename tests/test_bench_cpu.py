"""bench.py on the CPU: --dump-outputs (the files, their dtypes, the 64 MB cap and the run-to-run identity of what is written),
what a plain run leaves to --full, and loading the native library from a tree built beforehand that is read-only to the user
who runs the benchmark.
The end-to-end runs use the TAL_BENCH_FAKE plumbing mode (segments workload, deterministic tensors in place of GPU work)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.conftest import ROOT


def _bench(tmp_path, out, *args):
    env = dict(os.environ, TAL_BENCH_FAKE="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "TAL_BENCH_BACKEND", "TORCHELASTIC_USE_AGENT_STORE"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "segments", "--segments", "3", "--seconds", "30",
           "--dump-outputs", str(tmp_path / out)] + list(args)
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def test_dump_outputs_are_the_same_whatever_the_step_count(tmp_path):
    a = _bench(tmp_path, "a", "--gpus", "1", "--steps", "2", "--warmup", "1")
    b = _bench(tmp_path, "b", "--gpus", "1", "--steps", "5", "--warmup", "0", "--passes", "1")
    assert (a["steps"], b["steps"]) == (2, 5) and a["ms_per_step"] > 0 and b["ms_per_step"] > 0
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) == ["feat.npy", "ids.npy"]
    tp = a["config"]["frames_per_step"] // 3
    tp = ((((tp - 21) // 2 + 1) - 21) // 2 + 1 - 21) // 2 + 1
    for name, dtype, shape in (("feat", np.float32, (3 * tp, 128)), ("ids", np.float64, (3 * tp, 1))):
        x, y = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert x.dtype == dtype and x.shape == shape
        np.testing.assert_array_equal(x, y)
    assert a["dump_outputs"]["arrays"]["feat"] == {"shape": [3 * tp, 128], "rows_of": 3 * tp}


def test_dump_outputs_of_two_ranks_match_one_rank(tmp_path):
    _bench(tmp_path, "one", "--gpus", "1", "--steps", "1", "--warmup", "0")
    _bench(tmp_path, "two", "--gpus", "2", "--steps", "1", "--warmup", "0")
    for name in ("feat", "ids"):
        np.testing.assert_array_equal(np.load(tmp_path / "one" / (name + ".npy")), np.load(tmp_path / "two" / (name + ".npy")))


def test_dump_outputs_cap_keeps_the_same_seeded_rows(tmp_path):
    import bench
    rows = 200_000
    feat = torch.arange(rows * 128, dtype=torch.float32).reshape(2, rows // 2, 128)      # 102 MB: over the cap
    ids = torch.arange(rows, dtype=torch.int32)
    tokens = np.arange(7, dtype=np.int64)
    got = bench.dump_outputs(str(tmp_path / "a"), {"feat": feat, "ids": ids, "tokens": tokens})
    again = bench.dump_outputs(str(tmp_path / "b"), {"feat": feat, "ids": ids, "tokens": tokens})
    assert got == again
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_BYTES
    f, i = np.load(tmp_path / "a" / "feat.npy"), np.load(tmp_path / "a" / "ids.npy")
    assert f.dtype == np.float32 and i.dtype == np.float64 and got["feat"]["rows_of"] == rows
    assert 0 < f.shape[0] < rows and f.shape[0] == i.shape[0]
    # the rows kept are sorted, distinct, and the same frames in both arrays
    np.testing.assert_array_equal(f[:, 0] / 128, i[:, 0])
    assert (np.diff(i[:, 0]) > 0).all()
    np.testing.assert_array_equal(f, np.load(tmp_path / "b" / "feat.npy"))
    # a small array is cut by the same fraction, never to nothing
    t = np.load(tmp_path / "a" / "tokens.npy")
    assert t.dtype == np.float64 and 1 <= t.shape[0] <= 7 and t.shape[1] == 1


LEGS = ("no_cpu_baseline", "no_prof", "no_exact_pass", "no_clip_latency", "no_per_rank_share", "no_decode_episode",
        "no_one_gpu_reference", "no_clock_sampler")


def test_plain_run_switches_every_other_leg_off(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert not a.full and all(getattr(a, k) for k in LEGS)
    assert (a.workload, a.steps, a.warmup, a.passes) == ("clip", 3, 1, 3)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--full"])
    a = bench.parse()
    assert a.full and not any(getattr(a, k) for k in LEGS)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-baseline"])
    a = bench.parse()
    assert a.no_cpu_baseline and not a.no_prof


def test_full_adds_legs_and_keeps_the_timed_steps(tmp_path):
    """--full adds what lies beside the headline (here: rank 0's solo pass over the same segments of a two-rank run); the
    line's headline fields and the dumped outputs of the timed steps are those of the plain run."""
    plain = _bench(tmp_path, "plain", "--gpus", "2", "--steps", "2", "--warmup", "1")
    full = _bench(tmp_path, "full", "--gpus", "2", "--steps", "2", "--warmup", "1", "--full")
    assert "one_gpu_same_workload" not in plain and "speedup_vs_one_gpu" not in plain
    assert full["one_gpu_same_workload"]["n_gpus"] == 1 and full["speedup_vs_one_gpu"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "n_gpus", "config"):
        assert plain[k] == full[k], k
    assert plain["ms_per_step"] > 0 and len(plain["ms_per_step_passes"]) == 3
    for name in ("feat", "ids"):
        np.testing.assert_array_equal(np.load(tmp_path / "plain" / (name + ".npy")), np.load(tmp_path / "full" / (name + ".npy")))


def _refuse(*a, **k):
    raise PermissionError(13, "Permission denied (read-only tree)")


def test_build_writes_nothing_when_the_library_is_fresh(monkeypatch):
    """A tree built beforehand (by another user, say) may be read-only to the one who runs the tests or the benchmark:
    build() of a fresh library creates no directory, opens no lock file and starts no compiler."""
    import __graft_entry__ as g
    g.build()
    monkeypatch.setattr(g, "open", _refuse, raising=False)
    monkeypatch.setattr(g.os, "makedirs", _refuse)
    monkeypatch.setattr(g.subprocess, "Popen", _refuse)
    monkeypatch.setattr(g.subprocess, "check_call", _refuse)
    g.build()


def test_bench_loads_a_fresh_library_when_build_cannot_take_its_lock(monkeypatch):
    """A build() that takes its lock file even with nothing to build (the form before the one above) raises
    PermissionError on such a tree: bench.py then loads the library as it is -- but never one older than its sources."""
    import __graft_entry__ as g
    import bench
    g.build()
    monkeypatch.setattr(g, "build", _refuse)
    bench.build_native()
    lib = os.path.join(ROOT, "tal_asrd_amd", "libtal_asrd_hip.so")
    mtime = os.path.getmtime
    monkeypatch.setattr(os.path, "getmtime", lambda p: mtime(p) - (1e6 if os.path.samefile(p, lib) else 0))
    with pytest.raises(PermissionError):
        bench.build_native()
