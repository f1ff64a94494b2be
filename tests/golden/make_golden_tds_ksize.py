"""Record fixtures from the reference's TDS encoder at kernel sizes other than 21.  BUILD-CONTAINER ONLY: needs the reference
tree (tests/golden/_refload.py).
  tds_ksize.npz        TDS(input_size=8, sizes=[8, 16, 24, 32], depths=[1, 1, 2], kernel_size=k) for k in {3, 11, 31} on x [2, 8, 300]
                       (keys tds_k{k}_x / _y); TDS(8, [8, 16, 24, 32], [0, 0, 0], kernel_size=8) on the same x (tds_k8_x / _y: even k,
                       resize convs only); TDSBlock(32, k, 8) for k in {5, 15} on x [2, 32, 60] (block_k{k}_x / _y)
  tds_ksize_keys.json  state_dict keys and shapes of TDS(80, [80, 800, 1120, 1440], [2, 3, 6], kernel_size=k) and TDSBlock(32, k, 8)
                       for k in {3, 15}
  sd_k15_30s.npz       the reference SDModel() with its encoder replaced by TDS(80, [80, 800, 1120, 1440], [2, 3, 6], kernel_size=15),
                       on the 30 s synthetic clip: the fields of make_golden._sd_fixture; a seed whose closest top-2 logit margin is
                       within 1e-4 is rejected and the next one tried
Weights: synth.fill_state_dict, as make_golden.py (the small modules' keys namespaced by the fixture key, e.g. "tds_k3.").

    python tests/golden/make_golden_tds_ksize.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import _refload  # noqa: E402
from tests.golden.make_golden import fill, rows, save, top2_margin  # noqa: E402
from tal_asrd_amd import synth  # noqa: E402

torch.set_grad_enabled(False)
MARGIN_MIN = 1e-4
SD_SIZES, SD_DEPTHS, SD_K = [80, 800, 1120, 1440], [2, 3, 6], 15


def small_fixtures(M):
    out = {}
    x = synth.synth_tensor("tds_ksize/x", (2, 8, 300), 1.0)
    for k, depths in ((3, [1, 1, 2]), (11, [1, 1, 2]), (31, [1, 1, 2]), (8, [0, 0, 0])):
        tds = fill(M.TDS(input_size=8, sizes=[8, 16, 24, 32], depths=depths, kernel_size=k), "tds_k%d." % k)
        out["tds_k%d_x" % k] = x
        out["tds_k%d_y" % k] = tds(torch.from_numpy(x)).numpy()
    xb = synth.synth_tensor("tds_ksize/xb", (2, 32, 60), 1.0)
    for k in (5, 15):
        blk = fill(M.TDSBlock(32, k, 8), "block_k%d." % k)
        out["block_k%d_x" % k] = xb
        out["block_k%d_y" % k] = blk(torch.from_numpy(xb)).numpy()
    save("tds_ksize", **out)


def keys(M):
    res = {}
    for k in (3, 15):
        res["TDS_k%d" % k] = [[n, list(v.shape)] for n, v in M.TDS(80, SD_SIZES, SD_DEPTHS, kernel_size=k).state_dict().items()]
        res["TDSBlock_k%d" % k] = [[n, list(v.shape)] for n, v in M.TDSBlock(32, k, 8).state_dict().items()]
    with open(os.path.join(HERE, "tds_ksize_keys.json"), "w") as f:
        json.dump(res, f, indent=0)
    print("wrote tds_ksize_keys.json")


def sd_fixture(M, name="sd_k15_30s", L=480000, seed0=1234, n_rows=8):
    """make_golden._sd_fixture for SDModel() with a kernel-size-15 encoder, with the margin rule over seeds seed0, seed0 + 1, ..."""
    model = M.SDModel()
    model.encoder = M.TDS(80, SD_SIZES, SD_DEPTHS, kernel_size=SD_K)
    model = fill(model)
    for seed in range(seed0, seed0 + 20):
        audio = synth.synth_audio_batch(1, L, seed)
        mel = model.extract_features(torch.from_numpy(audio))
        enc = model.encode_features(mel)
        eo = enc["encoder_out"]
        logits = model.decode(enc)
        margin = top2_margin(logits)
        if margin.min() > MARGIN_MIN:
            break
        print("%s: seed %d rejected (closest top-2 margin %.2e)" % (name, seed, margin.min()))
    else:
        raise RuntimeError("%s: no seed with every top-2 margin above %g" % (name, MARGIN_MIN))
    ids = logits.argmax(-1)
    r = rows(ids.shape[1], n_rows)
    mr = rows(mel.shape[1], 16)
    save(name, audio_seed=seed, audio_len=L, batch=1, kernel_size=SD_K,
         mel_rows=mr, mel_sample=mel[:, mr].numpy(), mel_sum=mel.double().sum(dim=(1, 2)).numpy(),
         mel_abs_sum=mel.double().abs().sum(dim=(1, 2)).numpy(),
         enc_rows=r, enc_sample=eo[:, r].numpy(), enc_chan_sum=eo.double().sum(dim=1).numpy(),
         feat=model.spk_embed_proj(eo).numpy().astype(np.float32),
         logit_rows=r, logit_sample=logits[:, r].numpy(),
         ids=ids.numpy().astype(np.int32), margin=margin.astype(np.float32),
         logit_max=logits.max(-1).values.numpy())
    print("%s: seed %d, closest top-2 margin %.3e" % (name, seed, margin.min()))


def main():
    M = _refload.load_reference().models
    small_fixtures(M)
    keys(M)
    sd_fixture(M)


if __name__ == "__main__":
    main()
