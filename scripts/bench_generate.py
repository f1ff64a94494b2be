"""System.generate, search="host" against search="device": ms per decode step at the batch shape of the windowed transcription
(tal/asr/transcribe.py:124-162: B windows of 30 s in one call), same process, the two modes alternating.

    python scripts/bench_generate.py [--windows 8] [--seconds 30] [--steps 64] [--reps 7] [--no-trace]

Cases: beam 1 and beam 3 without the speaker head, beam 1 with it; no terminate token, so every call runs all its steps.
A call is encode + steps; the encoder is timed on its own (same input, same alternation) and subtracted, so
ms/step = (median call - median encode) / steps.  Prints the raw medians too, whether the two modes return identical outputs
(sequences equal, speaker logits torch.equal), and -- unless --no-trace -- the device activities (kernels, copies) per step of
each mode, counted by torch.profiler in a separate short run."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import __graft_entry__ as g

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=8)
ap.add_argument("--seconds", type=float, default=30.0)
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--no-trace", action="store_true")
args = ap.parse_args()

g.build()
from tal_asrd_amd import ASRModel, synth
from tal_asrd_amd.system import System

assert torch.cuda.is_available(), "bench_generate.py measures on the GPU"
dev = torch.device("cuda:0")
m = ASRModel("2x", num_speakers=6008, vocab_size=10000, use_speaker_head=True)
sd = synth.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
own = m.state_dict()
for k, v in sd.items():
    own[k] = torch.from_numpy(v.copy())
m.load_state_dict(own)
m.to(dev)
B, L = args.windows, int(args.seconds * 16000)
audio = torch.from_numpy(synth.synth_audio_batch(B, L, 4242)).to(dev)
lens = torch.tensor([L] * B)
prime = torch.zeros(B, 1, dtype=torch.long, device=dev)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def same(a, b):
    for xs, ys in zip(a, b):
        for x, y in zip(xs, ys):
            if (x is None) != (y is None) or (x is not None and not torch.equal(x, y)):
                return False
    return True


def activities(fn, steps):
    """Device activities per step of one call: (kernels, copies), by torch.profiler; None when the profiler gives nothing."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev_type = getattr(torch.autograd, "DeviceType", None)
        ev = [e for e in prof.events() if dev_type is not None and e.device_type == dev_type.CUDA]
        if not ev:
            return None
        copies = sum(1 for e in ev if "memcpy" in e.name.lower() or "memset" in e.name.lower())
        return (len(ev) - copies) / steps, copies / steps
    except Exception as e:      # noqa: BLE001 -- measurement aid only
        print("  (no activity count: %r)" % (e,))
        return None


print("System.generate: %d windows of %.0f s, %d steps, no terminate token; %d alternating repetitions after one warm-up call per mode"
      % (B, args.seconds, args.steps, args.reps))
for beam, spk in ((1, False), (3, False), (1, True)):
    sys_ = System(m, spk_weight=1.0 if spk else 0.0)

    def call(search, steps=args.steps):
        return sys_.generate(audio, prime, lens, length=steps, beam_size=beam, force_half=True, search=search)

    def encode():
        return m.encode(audio.half(), lens)
    outs = {s: call(s) for s in ("host", "device")}          # warm-up: every shape of the timed window
    identical = same(outs["host"], outs["device"])
    t = {"host": [], "device": [], "encode": []}
    for _ in range(args.reps):
        for s in ("host", "device"):
            t[s].append(timed(lambda: call(s))[0])
        t["encode"].append(timed(encode)[0])
    med = {k: statistics.median(v) for k, v in t.items()}
    per = {s: (med[s] - med["encode"]) / args.steps for s in ("host", "device")}
    print("beam %d%s: host %.3f ms/step, device %.3f ms/step (x%.2f); outputs identical: %s"
          % (beam, " + speaker head" if spk else "", per["host"], per["device"], per["host"] / per["device"], identical))
    print("  medians [min .. max] ms: " + ", ".join("%s %.1f [%.1f .. %.1f]" % (k, med[k], min(t[k]), max(t[k])) for k in ("host", "device", "encode")))
    if not args.no_trace:
        short = 8
        for s in ("host", "device"):
            full = activities(lambda: call(s, short), 1)
            enc = activities(encode, 1)
            if full and enc:
                print("  %s: %.1f kernels + %.1f copies / memsets per step (encoder's subtracted)"
                      % (s, (full[0] - enc[0]) / short, (full[1] - enc[1]) / short))
