"""The any-k grouped convs (csrc/gconv_general.hip) on the per-stage shapes of a 1-hour clip, in one process (HIP events):
  1. k = 21: the any-k kernel against the specialised VALU kernels (gconv_kernel / gconv_s2_c1_kernel) and the fp16x3 matrix-core kernels;
  2. the any-k kernel alone at k in {11, 15, 21, 31, 63} (cost against k);
  3. SDModel.speaker_ids on one hour with a k = 15 encoder against the default k = 21 one.
    python scripts/bench_gconv_general.py [--reps N]
Results: profiles/gconv_general_shapes.txt."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__ as g  # noqa: E402

g.build()
from tal_asrd_amd import ops, synth  # noqa: E402
from tal_asrd_amd.models import SDModel, TDS  # noqa: E402

dev = torch.device("cuda:0")
G = 80
# (label, stride, C_in / G, C_out / G, input frames of the 1-hour clip at that stage)
SHAPES = (("s2 1->10", 2, 1, 10, 360001), ("s2 10->14", 2, 10, 14, 179991), ("s2 14->18", 2, 14, 18, 89986),
          ("res 10", 1, 10, 10, 179991), ("res 14", 1, 14, 14, 89986), ("res 18", 1, 18, 18, 44983))


def timeit(fn, reps):
    """median per-call time (ms) of `reps` calls, each between its own pair of events, after two warm-up calls"""
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def conv_case(stride, cig, cog, T, k):
    x = torch.rand(1, T, G * cig, device=dev) * 2 - 1
    w = (torch.rand(G * cog, cig, k, device=dev) * 2 - 1) / (cig * k) ** 0.5
    b = torch.rand(G * cog, device=dev) * 0.2 - 0.1
    return x, w, b, ops.pack_gconv_weight(w, G)


def macs(stride, cig, cog, T, k):
    t_out = (T - k) // 2 + 1 if stride == 2 else T
    return t_out * G * cog * cig * k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    print("device: %s" % torch.cuda.get_device_name(0))
    print("\n1. k = 21, 1-hour per-stage shapes: median ms per launch (%d reps)" % args.reps)
    print("%-10s %10s %10s %10s %8s %10s" % ("shape", "any-k", "VALU", "fp16x3", "any/VALU", "any TFLOP/s"))
    for label, stride, cig, cog, T in SHAPES:
        x, w, b, wp = conv_case(stride, cig, cog, T, 21)
        if stride == 2:
            t_new = timeit(lambda: ops.gconv_s2_k(x, wp, b, G * cog, G, 21), args.reps)
            t_valu = timeit(lambda: ops.gconv_s2(x, wp, b, G * cog, G), args.reps)
            wf = ops.pack_gconv_f16x3_weight(w, G, stride=2)
            t_mfma = timeit(lambda: ops.gconv_s2_f16x3(x, wf, b, G * cog, G), args.reps) if wf is not None else float("nan")
        else:
            t_new = timeit(lambda: ops.gconv_res_k(x, wp, b, 0.25, G, 21), args.reps)
            t_valu = timeit(lambda: ops.gconv_res(x, wp, b, 0.25, G), args.reps)
            wf = ops.pack_gconv_f16x3_weight(w, G)
            t_mfma = timeit(lambda: ops.gconv_res_f16x3(x, wf, b, 0.25, G), args.reps) if wf is not None else float("nan")
        print("%-10s %10.3f %10.3f %10.3f %8.2f %10.1f" % (label, t_new, t_valu, t_mfma, t_new / t_valu,
                                                         2.0 * macs(stride, cig, cog, T, 21) / t_new / 1e9))
        del x, w, b, wp
        torch.cuda.empty_cache()
    ks = (11, 15, 21, 31, 63)
    print("\n2. the any-k kernel against k: median ms per launch (ps per multiply-add in brackets)")
    print("%-10s " % "shape" + " ".join("%16s" % ("k=%d" % k) for k in ks))
    for label, stride, cig, cog, T in SHAPES:
        row = []
        for k in ks:
            x, w, b, wp = conv_case(stride, cig, cog, T, k)
            if stride == 2:
                t = timeit(lambda: ops.gconv_s2_k(x, wp, b, G * cog, G, k), args.reps)
            else:
                t = timeit(lambda: ops.gconv_res_k(x, wp, b, 0.25, G, k), args.reps)
            row.append("%7.3f (%4.2f)" % (t, t * 1e9 / macs(stride, cig, cog, T, k)))
            del x, w, b, wp
        torch.cuda.empty_cache()
        print("%-10s " % label + " ".join("%16s" % r for r in row))
    print("\n3. SDModel.speaker_ids on one hour of audio: median ms per call (%d reps)" % max(5, args.reps // 4))
    audio = torch.from_numpy(synth.synth_audio_batch(1, 16000 * 3600, 1234)).to(dev)
    for k in (21, 15):
        m = SDModel()
        if k != 21:
            m.encoder = TDS(80, [80, 800, 1120, 1440], [2, 3, 6], kernel_size=k)
        own = m.state_dict()
        for name, v in synth.fill_state_dict({n: tuple(t.shape) for n, t in own.items()}).items():
            own[name] = torch.from_numpy(v.copy())
        m.load_state_dict(own)
        m = m.to(dev).eval()
        with torch.no_grad():
            t = timeit(lambda: m.speaker_ids(audio), max(5, args.reps // 4))
        print("k=%d: %.2f ms" % (k, t))
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
