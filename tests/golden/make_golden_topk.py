"""Record tests/golden/sd_30s_topk.npz from the reference's OWN SDModel (build container only):

    python tests/golden/make_golden_topk.py

The sd_30s waveform (make_golden.py's: synth_audio_batch(1, 480000, 1234)) through the reference model with the synthetic weights;
per encoder frame the top-8 speaker ids of its fp32 logits, their log-softmax values and the row's log-sum-exp evaluated in
float64, and the smallest adjacent gap among the top `k_ids` + 1 logits.  `k_ids` says how many ids a test may compare: 4 when at
least 90 % of the rows have that gap above 2e-3 (twice the project's logit tolerance), else 2.  The fixture is data; no reference
source is stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden._refload import load_reference  # noqa: E402
from tests.golden.make_golden import fill, save  # noqa: E402
from tal_asrd_amd import synth  # noqa: E402

torch.set_grad_enabled(False)
GAP = 2e-3          # 2 x LOGIT_TOL of the GPU tests


def main():
    ns = load_reference()
    model = fill(ns.models.SDModel())
    audio = torch.from_numpy(synth.synth_audio_batch(1, 480000, 1234))
    enc = model.encode_features(model.extract_features(audio), None)
    logits = model.decode(enc)[0].double()                          # [T', 6008]: the reference's fp32 logits, widened
    lse = torch.logsumexp(logits, dim=-1)
    top = torch.topk(logits, 9, dim=-1)
    # torch.topk leaves the order of equal values open: the rule is ascending index, so a tie inside the top 9 is refused
    assert bool((top.values[:, :-1] > top.values[:, 1:]).all()), "equal logits among the top 9 of a row"
    gaps = top.values[:, :-1] - top.values[:, 1:]
    k_ids = 4
    if float((gaps[:, :4].min(dim=1).values > GAP).double().mean()) < 0.9:
        k_ids = 2
    min_gap = gaps[:, :k_ids].min(dim=1).values
    share = float((min_gap > GAP).double().mean())
    assert share >= 0.9, "only %.1f %% of the rows have their top-%d gaps above %g" % (100 * share, k_ids + 1, GAP)
    print("k_ids=%d: %.1f %% of %d rows have every gap among the top %d above %g" % (k_ids, 100 * share, logits.shape[0], k_ids + 1, GAP))
    save("sd_30s_topk", ids=top.indices[:, :8].numpy().astype(np.int32), logp=(top.values[:, :8] - lse[:, None]).numpy(),
         lse=lse.numpy(), min_gap=min_gap.numpy().astype(np.float32), k_ids=k_ids, audio_seed=1234, audio_len=480000)


if __name__ == "__main__":
    main()
