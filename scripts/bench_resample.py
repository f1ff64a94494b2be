"""Timings of tal_resample_fwd for profiles/resample_shapes.txt: per shape the median of 9 passes of 5 calls after 3 warm-up calls
(device events), bytes moved and GB/s, the conv1d-per-phase formulation on the same inputs, and what the resample adds to a 1-hour
SDModel.speaker_ids call.  Prints one JSON line per row; --out FILE also writes them to a file."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tal_asrd_amd import Resample, SDModel, synth  # noqa: E402
from tests import _resample_ref as R  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, calls=5, passes=9, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return statistics.median(out), min(out), max(out)


rows = []
for name, orig, sec, dtype in [("1h 44.1k int16", 44100, 3600, torch.int16), ("1h 48k fp32", 48000, 3600, torch.float32),
                               ("5min 44.1k int16", 44100, 300, torch.int16), ("30s 44.1k int16", 44100, 30, torch.int16),
                               ("5min 48k fp32", 48000, 300, torch.float32), ("30s 48k fp32", 48000, 30, torch.float32),
                               ("1h 8k int16", 8000, 3600, torch.int16), ("5min 16001 fp32 (L2 form)", 16001, 300, torch.float32)]:
    L = orig * sec
    g = torch.Generator(device=dev).manual_seed(1)
    if dtype == torch.int16:
        x = torch.randint(-32768, 32768, (1, L), generator=g, device=dev, dtype=torch.int16)
        xf = x.to(torch.float32) * 2.0 ** -15
    else:
        x = torch.rand(1, L, generator=g, device=dev) * 2 - 1
        xf = x
    rs = Resample(orig, 16000)
    n = rs.num_samples(L)
    med, lo, hi = timed(lambda: rs(x))
    nbytes = L * x.element_size() + n * 4
    row = {"case": name, "L_in": L, "n_out": n, "ms": med, "ms_min": lo, "ms_max": hi, "bytes": nbytes, "GBps": nbytes / med / 1e6}
    if orig != 16001:
        y = rs(x)
        yt = R.resample_torch(xf, orig, 16000)
        row["max_abs_diff_vs_conv1d"] = float((y - yt).abs().max())
        del y, yt
        tm, tlo, thi = timed(lambda: R.resample_torch(xf, orig, 16000), calls=2, passes=5, warm=1)
        row.update({"conv1d_ms": tm, "ratio": tm / med})
    rows.append(row)
    print(json.dumps(row), flush=True)
    del x, xf

# what the resample adds to a 1-hour speaker_ids call
model = SDModel()
shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
sd = synth.fill_state_dict(shapes)
own = model.state_dict()
for k, v in sd.items():
    own[k] = torch.from_numpy(v.copy())
model.load_state_dict(own)
model.to(dev)
a16 = torch.from_numpy(synth.synth_audio_batch(1, 3600 * 16000, 1)).to(dev)
a44 = torch.from_numpy(np.round(synth.synth_audio_batch(1, 3600 * 44100, 1) * 32767).astype(np.int16)).to(dev)
with torch.no_grad():
    t16 = timed(lambda: model.speaker_ids(a16), calls=3, passes=7, warm=2)
    t44 = timed(lambda: model.speaker_ids(a44, sample_rate=44100), calls=3, passes=7, warm=2)
    t16b = timed(lambda: model.speaker_ids(a16), calls=3, passes=7, warm=2)
row = {"case": "speaker_ids 1h", "ms_16k_fp32": t16[0], "ms_16k_fp32_again": t16b[0], "ms_44k1_int16_resampled": t44[0],
       "added_ms": t44[0] - (t16[0] + t16b[0]) / 2}
print(json.dumps(row), flush=True)
rows.append(row)
if "--out" in sys.argv:
    json.dump(rows, open(sys.argv[sys.argv.index("--out") + 1], "w"), indent=1)
