"""Times the general log-mel front-end (csrc/logmel_general.hip) on one hour of audio per shape, and in the same process the
two existing forms on the default shape (logmel_mfma = 0 / 1).  Each timed call is log-mel plus the mean subtraction; device
events, warm-up calls first, the median of --reps calls reported.  Also, for information, the 5-minute SDModel(n_mels) call.

    python scripts/bench_logmel_general.py [--reps 7] [--no-sd] [--forms default|all] [--sd-only N_MELS]

--forms default: the three forms of the default shape and the 48 kHz / 128-mel shape only (counter passes);
--sd-only N: only the SDModel(n_mels=N) timing (one kernel trace per mel count).
dft_gflop is the floor of the folded float64 DFT, T * 2 * (N/2) * n_bins * 2.  floor_tflops = that floor / time, given for the
matrix-core forms only: the fast transform (default form) does a different, O(N log N), amount of arithmetic.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-sd", action="store_true")
    ap.add_argument("--forms", choices=("all", "default"), default="all")
    ap.add_argument("--sd-only", type=int, default=0)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from tal_asrd_amd import LogMelSpec, SDModel, ops, synth, _native as N
    dev = torch.device("cuda:0")
    rows = []

    def run(label, sr, n_mels, general=False, mfma=None):
        m = LogMelSpec(sr=sr, n_mels=n_mels).to(dev)
        win, fb, hop = m.mel_transform.spectrogram.window, m.mel_transform.mel_scale.fb, m.mel_transform.hop_length
        n_fft = win.shape[0]
        N.set_option("logmel_general", 1 if general else 0)
        plan = ops.logmel_plan(win, fb, hop=hop)
        N.set_option("logmel_general", 0)
        if mfma is not None:
            N.set_option("logmel_mfma", mfma)
        L = sr * 3600
        x = (torch.rand(1, L, generator=torch.Generator(device=dev).manual_seed(1), device=dev) - 0.5) * 0.6
        ms = timed(lambda: ops.logmel(plan, x, eps=m.eps, subtract_mean=True), args.reps)
        N.set_option("logmel_mfma", 0)
        T = 1 + L // hop
        nb = n_fft // 2 + 1
        floor = T * 2 * (n_fft / 2) * nb * 2            # FLOP of the folded float64 DFT: T . 2 . (N/2) . n_bins . 2
        r = {"form": label, "sr": sr, "n_mels": n_mels, "n_fft": n_fft, "hop": hop, "frames": T, "ms_per_hour": round(ms, 4),
             "dft_gflop": round(floor / 1e9, 1), "floor_tflops": None if label.startswith("fft") else round(floor / ms / 1e9, 1),
             "kind": type(plan).__name__}
        rows.append(r)
        print(json.dumps(r), flush=True)
        del x

    if not args.sd_only:
        run("fft (default form, logmel_mfma=0)", 16000, 80, mfma=0)
        run("mfma (logmel_mfma=1)", 16000, 80, mfma=1)
        run("general forced (logmel_general=1)", 16000, 80, general=True)
        shapes = ((48000, 128),) if args.forms == "default" else ((16000, 40), (16000, 128), (8000, 80), (22050, 80), (48000, 128))
        for sr, nm in shapes:
            run("general", sr, nm)
        by = {r["form"]: r["ms_per_hour"] for r in rows}
        ratio = by["general forced (logmel_general=1)"] / by["mfma (logmel_mfma=1)"]
        print(json.dumps({"gate": "general forced / logmel_mfma=1 on the default shape", "ratio": round(ratio, 3), "limit": 1.25,
                          "met": ratio <= 1.25}), flush=True)

    if args.sd_only or not args.no_sd:
        for nm in ((args.sd_only,) if args.sd_only else (80, 40, 64)):
            model = SDModel(n_mels=nm)
            own = model.state_dict()
            shapes = {k: tuple(v.shape) for k, v in own.items() if "mel_transform" not in k}
            for k, v in synth.fill_state_dict(shapes).items():
                own[k] = torch.from_numpy(v.copy())
            model.load_state_dict(own)
            model.to(dev)
            x = torch.from_numpy(synth.synth_audio_batch(1, 16000 * 300, 5)).to(dev)
            with torch.no_grad():
                ms = timed(lambda: model.speaker_ids(x), args.reps, warm=2)
            print(json.dumps({"model": "SDModel(n_mels=%d).speaker_ids" % nm, "audio_s": 300, "ms": round(ms, 3)}), flush=True)


if __name__ == "__main__":
    main()
