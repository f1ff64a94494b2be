"""Speaker turns on the device (ops.speaker_turns, SDModel.speaker_turns) next to the host route a caller had before.

    python scripts/bench_speaker_turns.py [--repeats 9] [--quick] [--out profiles/speaker_turns.txt]

Two shapes: one 1-hour clip (44,983 encoder frames) and the 64 x 5 min batch (64 x 3,733 = 238,912 frames, one item per row).
SDModel with seeded synthetic weights on seeded synthetic audio.  Per shape:
  ops.speaker_turns           device events round one call (11 + 5 launches and the one read-back of the turn count; the GPU idles
                              during the read-back and the wrapper's host work, and that is inside the figure), smooth = 6,
                              min_frames = 13, with embeddings and frame labels; on the model's own ids and on a seeded sticky chain
                              over 8 speakers (mean run about 4 s) that stands in for trained weights
  read-back                   wall clock of one 16-byte device-to-host read on an idle stream: what the single read of the turn count
                              costs at least, and its share of the call
  SDModel.speaker_turns       wall clock with a synchronise, next to SDModel.speaker_ids on the same input: the difference is what the
                              turns add to a diarization call
  host route                  ids.cpu() + feat.cpu() + the NumPy model of the tests (tests/_turns_ref.py: mode filter, runs, minimum
                              duration, float64 segment mean) on the same box, once; its integer outputs are checked equal to the
                              device's
Device events / wall clocks: `repeats` calls one by one behind 2 untimed ones, median [min .. max].
--quick: the 1-hour shape only, no host route."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g.build()
    from tal_asrd_amd import SDModel, ops, synth
    from tests import _turns_ref as R
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def stats(out):
        return statistics.median(out), min(out), max(out)

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
        return stats(out)

    def wall(fn, warm=2):
        for _ in range(warm):
            fn()
        out = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
        return stats(out)

    model = SDModel()
    sd = synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    own = model.state_dict()
    for k, v in sd.items():
        own[k] = torch.from_numpy(v.copy())
    model.load_state_dict(own)
    model.to(dev)
    num_ids = model.spk_logit_proj.weight.shape[0]
    tile, _ = ops.speaker_turns_tile()
    say("speaker turns on %s: tiles of %d frames, segment-mean chunks of %d rows, smooth = 6, min_frames = 13"
        % (torch.cuda.get_device_name(0), tile, ops.SEGMENT_MEAN_CHUNK))
    say("ms: median [min .. max] of %d calls" % args.repeats)
    word = torch.zeros(2, dtype=torch.int64, device=dev)
    rb = wall(lambda: word.tolist())
    say("one 16-byte read-back on an idle stream (wall)      %8.3f  [%8.3f .. %8.3f]" % rb)
    shapes = [("1 hour", 1, 3600)] + ([] if args.quick else [("64 x 5 min", 64, 300)])
    for name, B, sec in shapes:
        audio = torch.cat([torch.from_numpy(synth.synth_audio_batch(1, sec * 16000, 1234 + i)) for i in range(B)]).to(dev)
        feat, ids = model.speaker_ids(audio)
        frames = ids.shape[-1]
        n = ids.numel()
        off = [b * frames for b in range(B + 1)]
        chain = torch.from_numpy(R.sticky_chain(n, 8, 1.0 - 1.0 / 50, 77)).to(dev)
        say()
        say("%s: %d item(s) x %d frames = %d frames, features [%d, %d]" % (name, B, frames, n, n, feat.shape[-1]))
        for what, x in (("model ids (synthetic weights)", ids), ("sticky chain, 8 speakers", chain)):
            res = ops.speaker_turns(x, num_ids, off, 6, 13, feat=feat, want_frames=True)
            raw_runs = int((x.reshape(-1)[1:] != x.reshape(-1)[:-1]).sum()) + 1
            say("  %s: %d raw runs -> %d turns" % (what, raw_runs, res.num_turns))
            med, lo, hi = timed(lambda: ops.speaker_turns(x, num_ids, off, 6, 13, feat=feat, want_frames=True))
            say("    ops.speaker_turns + embeddings (device events)  %8.3f  [%8.3f .. %8.3f]   read-back share >= %.0f %%"
                % (med, lo, hi, 100 * rb[0] / med))
            med, lo, hi = timed(lambda: ops.speaker_turns(x, num_ids, off, 6, 13))
            say("    ops.speaker_turns, no embeddings, no frames     %8.3f  [%8.3f .. %8.3f]" % (med, lo, hi))
        t_ids = wall(lambda: model.speaker_ids(audio))
        t_turns = wall(lambda: model.speaker_turns(audio))
        say("  SDModel.speaker_ids (wall)                          %8.3f  [%8.3f .. %8.3f]" % t_ids)
        say("  SDModel.speaker_turns (wall)                        %8.3f  [%8.3f .. %8.3f]   turns add %.3f ms (medians)"
            % (t_turns + (t_turns[0] - t_ids[0],)))
        if not args.quick:
            res = ops.speaker_turns(ids, num_ids, off, 6, 13, feat=feat, want_frames=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids_h, feat_h = ids.cpu().numpy().reshape(-1), feat.cpu().numpy().reshape(n, -1)
            t1 = time.perf_counter()
            ref = R.speaker_turns(ids_h, num_ids, off, 6, 13)
            t2 = time.perf_counter()
            ranges = []
            for b in range(B):
                for k in range(int(ref.offsets[b]), int(ref.offsets[b + 1])):
                    ranges.append((off[b] + int(ref.start[k]), off[b] + int(ref.end[k])))
            emb = R.segment_mean64(feat_h, ranges)
            t3 = time.perf_counter()
            same = all(np.array_equal(getattr(res, f).cpu().numpy(), getattr(ref, f))
                       for f in ("offsets", "start", "end", "label", "purity", "frame_labels"))
            err = float(np.abs(res.embed.cpu().numpy() - emb).max()) if len(ranges) else 0.0
            say("  host route, once: copies %.1f ms + turns %.1f ms + float64 means %.1f ms = %.1f ms; integer outputs %s, max |embed - float64| %.2e"
                % (1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), 1e3 * (t3 - t0), "IDENTICAL" if same else "DIFFERENT", err))
            assert same
        del audio, feat, ids
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
