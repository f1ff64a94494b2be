"""Per-row top-k speaker posteriors (tal_spk_topk_fwd) on the 1-hour shape, both forms, next to the arg-max head they sit beside.

    python scripts/bench_head_topk.py [--passes 7] [--iters 10] [--rows 44983] [--sweep] [--out profiles/head_topk.txt]

One process; every pass times every variant once (device events around `iters` back-to-back calls behind 2 untimed ones), the
variants in the same order pass after pass so that clock drift spreads over all of them; the figure of a variant is the median of
its passes.  The shader clock is sampled over the whole measurement by bench.py's child-process sampler.  Variants:
  fused k = 1, 4, 8   the A-stationary kernel (option head_topk_form=2)
  generic k = 1, 4, 8 dense layer into the workspace + row kernel (head_topk_form=1)
  arg-max             ops.sd_head(want_logits=False): 1440 -> 128 embedding layer + the arg-max kernel (the yardstick: it includes
                      the embedding layer, listed by itself as "features only")
--sweep times both forms at k = 8 over a ladder of row counts: the auto threshold of the dispatch is the row count from which the
fused form is the faster one."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import __graft_entry__ as g  # noqa: E402

S, E = 6008, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rows", type=int, default=44983)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g.build()
    from bench import ClockSampler
    from tal_asrd_amd import _native as N, ops
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1)
    wl = (torch.randn(S, E, generator=gen) / 11).to(dev)
    bl = torch.randn(S, generator=gen).to(dev)
    we = (torch.randn(E, 1440, generator=gen) / 38).to(dev)
    be = torch.randn(E, generator=gen).to(dev)

    def timed(fn):
        for _ in range(2):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters

    def topk(feat, k, form):
        def run():
            N.set_option("head_topk_form", form)
            try:
                return ops.spk_topk(feat, wl, bl, k)
            finally:
                N.set_option("head_topk_form", 0)
        return run

    def measure(variants):
        times = {name: [] for name, _ in variants}
        for _ in range(args.passes):
            for name, fn in variants:
                times[name].append(timed(fn))
        return {name: (statistics.median(v), min(v), max(v)) for name, v in times.items()}

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    sampler = ClockSampler(0)
    t0 = time.time()
    M = args.rows
    feat = torch.randn(M, E, generator=gen).to(dev)
    x = torch.randn(M, 1440, generator=gen).to(dev)
    variants = [("fused   k=%d" % k, topk(feat, k, 2)) for k in (1, 4, 8)] + [("generic k=%d" % k, topk(feat, k, 1)) for k in (1, 4, 8)]
    variants.append(("arg-max head (sd_head, ids only)", lambda: ops.sd_head(x, we, be, wl, bl, want_logits=False, want_ids=True)))
    variants.append(("features only (sd_head)", lambda: ops.sd_head(x, we, be, wl, bl, want_logits=False, want_ids=False)))
    res = measure(variants)
    say("tal_spk_topk_fwd, M = %d rows, S = %d, E = %d; %d passes x %d calls, ms per call: median [min .. max]" % (M, S, E, args.passes, args.iters))
    flop = 2.0 * M * S * E
    for name, _ in variants:
        med, lo, hi = res[name]
        say("  %-34s %8.3f  [%7.3f .. %7.3f]%s" % (name, med, lo, hi, "   %5.1f TFLOP/s of the %d GFLOP" % (flop / med / 1e9, flop / 1e9)
                                                   if name[:5] in ("fused", "gener") else ""))
    a, f = res["arg-max head (sd_head, ids only)"][0], res["features only (sd_head)"][0]
    say("  arg-max kernel alone (difference of the last two): %.3f ms" % (a - f))
    # agreement at the size timed
    i2, p2, l2 = topk(feat, 8, 2)()
    i1, p1, l1 = topk(feat, 8, 1)()
    say("  forms agree at k = 8: ids equal on %.4f %% of rows, max |logp diff| %.2e, max |lse diff| %.2e"
        % (100.0 * float((i1 == i2).all(dim=1).float().mean()), float((p1 - p2).abs().max()), float((l1 - l2).abs().max())))
    if args.sweep:
        say()
        say("row-count sweep at k = 8, ms per call (median of %d passes)" % args.passes)
        say("  %8s %10s %10s   faster" % ("rows", "fused", "generic"))
        for rows in (128, 256, 512, 1024, 2048, 3751, 8192, 16384):
            fr = feat[:rows].contiguous()
            r = measure([("fused", topk(fr, 8, 2)), ("generic", topk(fr, 8, 1))])
            say("  %8d %10.3f %10.3f   %s" % (rows, r["fused"][0], r["generic"][0], "fused" if r["fused"][0] < r["generic"][0] else "generic"))
    t1 = time.time()
    sampler.close()
    clk = sampler.window(t0, t1)
    say()
    say("shader clock over the measurement: %s" % ("mean %.0f MHz, min %.0f MHz, socket power %.0f W (%d samples)"
        % (clk["sclk_mhz"], clk["sclk_mhz_min"], clk["power_w"] or 0.0, clk["samples"]) if clk.get("sclk_mhz") else "not sampled (%s)" % clk.get("unavailable")))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
