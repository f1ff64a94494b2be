"""WER / WDER scoring on the device (ops.edit_align, wder.calculate_wder(backend="device")) next to the host routines.

    python scripts/bench_edit_align.py [--repeats 7] [--sizes 1000,3000,10000] [--batch 8] [--host-sizes 1000,3000]
                                       [--quick] [--out profiles/edit_align.txt]

Seeded synthetic transcripts: a reference of `words` ids over a 5000-word vocabulary, the hypothesis a copy with about 15 %
substitutions, three block deletions and three block insertions (1 % of the length each); speaker labels change every 5 - 40 words
(4 reference speakers, 5 hypothesis speakers).  Per size, one pair (and a batch of --batch pairs at the largest size):
  distance only      ops.edit_align(want_path=False)                  the sweep of D alone
  path               ops.edit_align()                                 both tables, back-pointers, traceback
  path + counts      ops.edit_align(labels)                           + the label count matrix
  calculate_wder     wder.calculate_wder(backend="device"), wall clock: word -> id dicts, uploads, the call, the copies back, scipy
Device events with a synchronise round `repeats` calls one by one behind 2 untimed ones: median [min .. max].  The event figures
include the wrapper's host work (per-pair workspace arithmetic, the descriptor upload), the GPU being idle meanwhile.
The yardstick is wder.calculate_wder(backend="host") -- the parent commit's routine, unchanged -- on the same pairs in the same
process, timed once per --host-sizes entry (and checked equal to the device tuple); beyond them its figure is the measured per-cell
rate of the largest timed size times the cell count, labelled as an extrapolation.
--quick: the largest size only, no host yardstick (for runs under a kernel tracer or with an ablation build in TAL_ASRD_LIB)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as g  # noqa: E402


def make_pair(words, seed):
    """-> (ref ids, hyp ids, ref labels, hyp labels)"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 5000, words)

    def turns(n, speakers):
        out = np.zeros(n, dtype=np.int64)
        i = 0
        while i < n:
            k = int(rng.integers(5, 41))
            out[i:i + k] = rng.integers(0, speakers)
            i += k
        return out

    ref_lab = turns(words, 4)
    hyp, hyp_lab = ref.copy(), (ref_lab + 1) % 5
    flip = rng.random(words) < 0.15
    hyp[flip] = rng.integers(0, 5000, int(flip.sum()))
    blk = max(1, words // 100)
    for k in range(3):        # block deletions, then block insertions, at seeded places
        at = int(rng.integers(0, hyp.size - blk))
        hyp, hyp_lab = np.delete(hyp, slice(at, at + blk)), np.delete(hyp_lab, slice(at, at + blk))
    for k in range(3):
        at = int(rng.integers(0, hyp.size))
        hyp = np.insert(hyp, at, rng.integers(0, 5000, blk))
        hyp_lab = np.insert(hyp_lab, at, np.full(blk, k % 5))
    return ref, hyp, ref_lab, hyp_lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default="1000,3000,10000")
    ap.add_argument("--host-sizes", default="1000,3000")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g.build()
    from tal_asrd_amd import ops, wder as W
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    sizes = [int(x) for x in args.sizes.split(",")]
    host_sizes = [] if args.quick else [int(x) for x in args.host_sizes.split(",") if x]
    if args.quick:
        sizes = sizes[-1:]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        for _ in range(2):
            fn()
        out = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return statistics.median(out), min(out), max(out)

    def wall(fn):
        fn()
        out = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(out), min(out), max(out)

    rows, cols = ops.edit_align_tile()
    say("edit-distance alignment on %s, tiles of %d rows x %d columns, library %s" % (torch.cuda.get_device_name(0), rows, cols,
                                                                                      os.environ.get("TAL_ASRD_LIB", "(in-tree)")))
    say("ms per call: median [min .. max] of %d calls" % args.repeats)
    host_rate = None
    cases = [(w, 1) for w in sizes] + ([(sizes[-1], args.batch)] if args.batch > 1 and not args.quick else [])
    for words, P in cases:
        pairs = [make_pair(words, 100 + p) for p in range(P)]
        # ids and labels on the device beforehand: the three ops.edit_align figures time the call, not the upload
        a = [torch.from_numpy(x[0].astype(np.int32)).to(dev) for x in pairs]
        b = [torch.from_numpy(x[1].astype(np.int32)).to(dev) for x in pairs]
        la = [torch.from_numpy(x[2].astype(np.int32)).to(dev) for x in pairs]
        lb = [torch.from_numpy(x[3].astype(np.int32)).to(dev) for x in pairs]
        cells = sum(len(x[0]) * len(x[1]) for x in pairs)
        res = ops.edit_align(a, b, la, lb, n_labels=(4, 5))
        res0 = ops.edit_align(a, b, want_path=False)
        say()
        say("%d pair(s) of %d x %d words (%.3g cells): %d launches per call, workspace %d bytes (distance only: %d launches, %d bytes)"
            % (P, len(pairs[0][0]), len(pairs[0][1]), cells, res.launches, res.workspace_bytes, res0.launches, res0.workspace_bytes))
        stats = res.stats.cpu().numpy()
        say("  pair 0: distance %d, %d steps (%d equal, %d replace)" % tuple(stats[0]))
        for name, fn in (("distance only", lambda: ops.edit_align(a, b, want_path=False)),
                         ("path", lambda: ops.edit_align(a, b)),
                         ("path + counts", lambda: ops.edit_align(a, b, la, lb, n_labels=(4, 5)))):
            med, lo, hi = timed(fn)
            say("  %-28s %9.3f  [%8.3f .. %8.3f]   %.3g cells/s" % (name, med, lo, hi, cells / med * 1e3))
        ref = [[(int(w), "s%d" % s) for w, s in zip(x[0], x[2])] for x in pairs]
        hyp = [[(int(w), int(s)) for w, s in zip(x[1], x[3])] for x in pairs]
        if P == 1:
            med, lo, hi = wall(lambda: W.calculate_wder(ref[0], hyp[0], backend="device"))
            say("  %-28s %9.3f  [%8.3f .. %8.3f]   wall clock, host work included" % ("calculate_wder(device)", med, lo, hi))
            if words in host_sizes:
                t0 = time.perf_counter()
                want = W.calculate_wder(ref[0], hyp[0])
                t_host = time.perf_counter() - t0
                got = W.calculate_wder(ref[0], hyp[0], backend="device")
                same = got[:4] == want[:4] and list(got[4]) == list(want[4]) and list(got[5]) == list(want[5])
                host_rate = t_host / cells
                say("  %-28s %9.1f  (one run; %.3f us per cell)   the device tuple is %s: wer %.6f wder %.6f"
                    % ("calculate_wder(host)", 1e3 * t_host, 1e6 * host_rate, "IDENTICAL" if same else "DIFFERENT", want[0], want[3]))
                assert same
            elif host_rate is not None:
                say("  %-28s %9.1f  EXTRAPOLATED: %.3f us per cell (measured at the largest timed size) x %.3g cells"
                    % ("calculate_wder(host)", 1e3 * host_rate * cells, 1e6 * host_rate, cells))
        else:
            med, lo, hi = wall(lambda: W._wder_device(list(zip(ref, hyp)), False, True))
            say("  %-28s %9.3f  [%8.3f .. %8.3f]   wall clock, all %d pairs in one call" % ("wder (device, batched)", med, lo, hi, P))
            if host_rate is not None:
                say("  %-28s %9.1f  EXTRAPOLATED: %.3f us per cell x %.3g cells, one host thread"
                    % ("calculate_wder(host) x %d" % P, 1e3 * host_rate * cells, 1e6 * host_rate, cells))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
