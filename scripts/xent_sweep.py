"""Teacher-forced scoring of the tied LM head without the logits (tal_lm_xent_fwd) against today's path on the same inputs.

    python scripts/xent_sweep.py [--passes 5] [--iters 10] [--limit 180] [--out profiles/lm_xent.txt]

Paths, per head shape (D, E0, V) and row count M (64 .. 16,384 target positions):
  today    decoder.lm_head over all positions ([M, V] logits) + decoder.log_softmax (a second [M, V]) + torch.gather
  generic  tal_lm_xent_fwd, option xent_form=1: the logits of <= 64 MiB worth of rows into the workspace, one wave per row reads them
  fused    tal_lm_xent_fwd, option xent_form=2 (E0 = 64 only): logits through registers, never stored
A last table does the same for the speaker head alone (tal_xent_rows_fwd at E = 128, 6,008 speakers, with bias).
Every (shape, path) pair runs in a process of its own under its own time limit; a child that fails or runs out of time ends the
sweep (nothing more is started on the device after it).  A child times each row count as the median of `passes` device-event windows of
`iters` back-to-back calls behind 2 untimed ones, and reports the peak extra device memory of one call (torch's allocator: the
workspaces and today's logits all come from it) and, for the two new paths, the largest difference from today's path's result.
The auto threshold of the dispatch (XENT_FUSED_FROM_ROWS_* in csrc/head_plan.h) is read off the table this prints."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((512, 64, 16008), (256, 64, 10000), (256, 0, 10000), (0, 128, 6008))       # D = 0: the speaker head alone (tal_xent_rows_fwd)
ROWS = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)
FORMS = {"generic": 1, "fused": 2}


def child(args):
    import torch
    import __graft_entry__ as g
    g.build()
    from tal_asrd_amd import _native as N, decoder, ops
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    D, E0, V = args.shape
    gen = torch.Generator().manual_seed(1)
    width = E0 or D
    model = SimpleNamespace(embed_size=E0, embedding=SimpleNamespace(weight=(torch.randn(V, width, generator=gen) / width ** 0.5).to(dev)))
    if E0 and D:
        model.embedding_proj = SimpleNamespace(weight=(torch.randn(D, E0, generator=gen) / D ** 0.5).to(dev))
    h_all = torch.randn(1, ROWS[-1], D, generator=gen).to(dev)
    t_all = torch.randint(0, V, (1, ROWS[-1]), generator=gen).to(dev)

    def today(h, t):
        return -decoder.log_softmax(decoder.lm_head(model, h)).gather(-1, t.unsqueeze(-1)).squeeze(-1)

    def new(h, t):
        return decoder.lm_xent(model, h, t)[0]

    if D == 0:
        # the speaker head behind speaker_head[0]: features [M, 128] against speaker_head[1] with its bias
        w, b = model.embedding.weight, torch.randn(V, generator=gen).to(dev)
        h_all = torch.randn(1, ROWS[-1], E0, generator=gen).to(dev)

        def today(h, t):        # noqa: F811
            return -decoder.log_softmax(ops.linear(h, w, b)).gather(-1, t.unsqueeze(-1)).squeeze(-1)

        def new(h, t):          # noqa: F811
            return ops.xent_rows(h, w, b, t)
    fn = today if args.path == "today" else new
    if args.path != "today":
        N.set_option("xent_form", FORMS[args.path])
    out = []
    for M in ROWS:
        h, t = h_all[:, :M].contiguous(), t_all[:, :M].contiguous()
        for _ in range(2):
            res = fn(h, t)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = fn(h, t)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        times = []
        for _ in range(args.passes):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn(h, t)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / args.iters)
        diff = None
        if args.path != "today":
            N.set_option("xent_form", 0)
            diff = float((res - today(h, t)).abs().max())
            N.set_option("xent_form", FORMS[args.path])
        out.append({"rows": M, "ms": statistics.median(times), "ms_min": min(times), "ms_max": max(times), "peak_bytes": int(peak), "diff": diff})
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--limit", type=int, default=180, help="seconds a (shape, path) child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=4, default=None, metavar=("D", "E0", "V", "PATH"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        args.shape, args.path = tuple(int(x) for x in args.child[:3]), args.child[3]
        return child(args)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def finish(code):
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return code

    say("tal_lm_xent_fwd against lm_head + log_softmax + gather; %d passes x %d calls, ms per call (median), peak extra device memory of a call"
        % (args.passes, args.iters))
    for D, E0, V in SHAPES:
        paths = ["today", "generic"] + (["fused"] if E0 in (64, 128) else [])
        res = {}
        for path in paths:
            cmd = [sys.executable, os.path.abspath(__file__), "--passes", str(args.passes), "--iters", str(args.iters), "--child", str(D), str(E0),
                   str(V), path]
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                say("(D, E0, V) = (%d, %d, %d), %s: no result within %d s -- the sweep ends here" % (D, E0, V, path, args.limit))
                return finish(1)
            got = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not got:
                say("(D, E0, V) = (%d, %d, %d), %s: exit status %d -- the sweep ends here\n%s" % (D, E0, V, path, p.returncode, p.stdout[-2000:]))
                return finish(1)
            res[path] = {r["rows"]: r for r in json.loads(got[0][7:])}
        say()
        say("(D, E0, V) = (%d, %d, %d)%s" % (D, E0, V, "   the speaker head alone: tal_xent_rows_fwd, E = 128, with bias, against ops.linear + log_softmax + gather"
                                             if not D else "" if E0 else "   no projection: the generic form only"))
        say("  %7s | %9s %9s %9s | %10s %10s %10s | %s" % ("rows", "today", "generic", "fused", "today MiB", "generic MiB", "fused MiB",
                                                           "fastest new path; max |nll - today's|"))
        for M in ROWS:
            ms = {p: res[p][M]["ms"] for p in paths}
            mem = {p: res[p][M]["peak_bytes"] / 2.0 ** 20 for p in paths}
            new = {p: ms[p] for p in paths if p != "today"}
            best = min(new, key=new.get)
            diff = max(res[p][M]["diff"] for p in new)
            say("  %7d | %9.3f %9.3f %9s | %10.1f %10.1f %10s | %-7s %.2fx today's; %.2e"
                % (M, ms["today"], ms["generic"], "%9.3f" % ms["fused"] if "fused" in ms else "-", mem["today"], mem["generic"],
                   "%10.1f" % mem["fused"] if "fused" in mem else "-", best, ms["today"] / new[best], diff))
    return finish(0)


if __name__ == "__main__":
    sys.exit(main())
