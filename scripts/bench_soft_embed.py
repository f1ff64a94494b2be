"""Softmax-weighted speaker embeddings (tal_soft_embed_fwd) on the 1-hour shape, both forms, next to the route a caller had before:
the materialised logits, torch.softmax and torch.matmul.

    python scripts/bench_soft_embed.py [--passes 5] [--iters 5] [--rows 44983] [--sweep] [--out profiles/soft_embed.txt]

One process; every pass times every variant once (device events around `iters` back-to-back calls behind 2 untimed ones), the
variants in the same order pass after pass so that clock drift spreads over all of them; the figure of a variant is the median of
its passes.  The shader clock is sampled over the whole measurement by bench.py's child-process sampler.  Variants, at
(E, D) = (128, 128) (the diarizer head: w = values = spk_logit_proj.weight, with its bias) and (64, 64) (the tied LM head's 6008
speaker columns: w = values = embedding.weight[10000:], no bias, on already projected rows):
  fused      the two-product kernel (option soft_embed_form=2)
  generic    dense layer into the workspace + row kernel + dense layer (soft_embed_form=1)
  baseline   (128) ops.sd_head(want_logits=True) + torch.softmax + torch.matmul, with "features only (sd_head)" listed beside it:
             the baseline includes the 1440 -> 128 embedding layer, the two forms start from its output;
             (64) ops.linear onto all 16008 columns + torch.softmax of the speaker columns + torch.matmul
--sweep times both forms over a ladder of row counts at both widths: the auto threshold of the dispatch (SOFT_FUSED_FROM_ROWS_* in
csrc/head_plan.h) is the smallest row count of the ladder from which the fused form is the faster one at every larger count.
The last section runs the case table of tests/_soft_embed_ref.py through both forms and prints the largest error-to-bound ratio."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import __graft_entry__ as g  # noqa: E402

S, V0 = 6008, 10000
PEAK_TFLOPS = 155.0         # fp32 matrix peak of the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rows", type=int, default=44983)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g.build()
    from bench import ClockSampler
    from tal_asrd_amd import _native as N, ops
    from tests import _soft_embed_ref as R
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1)
    wl = (torch.randn(S, 128, generator=gen) / 11).to(dev)
    bl = torch.randn(S, generator=gen).to(dev)
    we = (torch.randn(128, 1440, generator=gen) / 38).to(dev)
    be = torch.randn(128, generator=gen).to(dev)
    emb = (torch.randn(V0 + S, 64, generator=gen) / 8).to(dev)
    spk_emb = emb[V0:]

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

    def soft(feat, w, b, form, grid=0, values=None):
        def run():
            N.set_option("soft_embed_form", form)
            N.set_option("soft_embed_grid", grid)
            try:
                return ops.soft_embed(feat, w, b, values, want_lse=True)
            finally:
                N.set_option("soft_embed_form", 0)
                N.set_option("soft_embed_grid", 0)
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
    feat = torch.randn(M, 128, generator=gen).to(dev)
    x = torch.randn(M, 1440, generator=gen).to(dev)
    t64 = torch.randn(M, 64, generator=gen).to(dev)

    def baseline128():
        _, logits, _ = ops.sd_head(x, we, be, wl, bl, want_logits=True, want_ids=False)
        return torch.matmul(torch.softmax(logits, dim=-1), wl)

    def baseline64():
        logits = ops.linear(t64, emb, None)
        return torch.matmul(torch.softmax(logits[:, V0:], dim=-1), spk_emb)

    for E, variants in ((128, [("fused", soft(feat, wl, bl, 2)), ("generic", soft(feat, wl, bl, 1)),
                               ("baseline: sd_head logits + softmax + matmul", baseline128),
                               ("features only (sd_head)", lambda: ops.sd_head(x, we, be, wl, bl, want_logits=False, want_ids=False))]),
                        (64, [("fused", soft(t64, spk_emb, None, 2)), ("generic", soft(t64, spk_emb, None, 1)),
                              ("baseline: all 16008 logits + softmax + matmul", baseline64)])):
        res = measure(variants)
        flop = 4.0 * M * S * E
        say("tal_soft_embed_fwd, M = %d rows, N = %d, E = D = %d, values = w; %d passes x %d calls, ms per call: median [min .. max]"
            % (M, S, E, args.passes, args.iters))
        for name, _ in variants:
            med, lo, hi = res[name]
            extra = ""
            if name in ("fused", "generic"):
                extra = "   %5.1f TFLOP/s of the %.0f GFLOP of the two products" % (flop / med / 1e9, flop / 1e9)
                if name == "fused":
                    extra += " = %.1f %% of the %.0f TFLOP/s fp32 matrix peak" % (100.0 * flop / med / 1e9 / PEAK_TFLOPS, PEAK_TFLOPS)
            say("  %-48s %8.3f  [%7.3f .. %7.3f]%s" % (name, med, lo, hi, extra))
        if E == 128:
            say("  baseline without its embedding layer (difference of the last two): %.3f ms"
                % (res["baseline: sd_head logits + softmax + matmul"][0] - res["features only (sd_head)"][0]))
        say("  fused %s generic at this shape (%.3f vs %.3f ms)" % ("beats" if res["fused"][0] < res["generic"][0] else "LOSES to",
                                                                  res["fused"][0], res["generic"][0]))
        a, b = variants[0][1](), variants[1][1]()
        say("  forms agree: max |out diff| %.2e, max |lse diff| %.2e" % (float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max())))
        say()
    # a separate values matrix (a second LDS image in the fused form)
    vals = torch.randn(S, 128, generator=gen).to(dev)
    res = measure([("fused", soft(feat, wl, bl, 2, values=vals)), ("generic", soft(feat, wl, bl, 1, values=vals))])
    say("separate values [%d, 128], M = %d: fused %.3f ms, generic %.3f ms" % (S, M, res["fused"][0], res["generic"][0]))
    if args.sweep:
        for E, f, w, b in ((128, feat, wl, bl), (64, t64, spk_emb, None)):
            say()
            say("row-count sweep at E = D = %d, values = w, ms per call (median of %d passes)" % (E, args.passes))
            say("  %8s %10s %10s   faster" % ("rows", "fused", "generic"))
            for rows in (128, 256, 512, 1024, 2048, 4096, 8192, 16384):
                fr = f[:rows].contiguous()
                r = measure([("fused", soft(fr, w, b, 2)), ("generic", soft(fr, w, b, 1))])
                say("  %8d %10.3f %10.3f   %s" % (rows, r["fused"][0], r["generic"][0], "fused" if r["fused"][0] < r["generic"][0] else "generic"))
    t1 = time.time()
    # accuracy: the GPU tests' case table through both forms, the largest |error| / bound
    worst, where = 0.0, None
    for name in sorted(R.CASES):
        feat_h, W_h, b_h, V_h, ref_alias, ref_sep = R.build(name)
        E = W_h.shape[1]
        fd, Wd, bd, Vd = (torch.from_numpy(a).to(dev) for a in (feat_h[:, :E].copy(), W_h, b_h, V_h))
        for ref, values in ((ref_alias, None), (ref_sep, Vd)):
            if ref is None:
                continue
            forms = [(1, 0)] + ([(2, gr) for gr in (0, 1, 2, 3, 7)] if E in R.FUSED_WIDTHS and ref.D == E else [])
            for form, grid in forms:
                out, lse = soft(fd, Wd, bd, form, grid, values)()
                bad = R.compare(ref, out.cpu().numpy(), lse.cpu().numpy())
                assert not bad, (name, form, grid, bad)
                ratio = R.error_ratio(ref, out.cpu().numpy())
                if ratio > worst:
                    worst, where = ratio, "%s, %s, form %d grid %d" % (name, "separate values" if ref.separate else "values = w", form, grid)
    say()
    say("largest |error| / bound over the case table of tests/_soft_embed_ref.py, both forms: %.4f (%s)" % (worst, where))
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
