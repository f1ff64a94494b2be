"""Record tests/golden/sd_30s_soft.npz and tests/golden/asr_soft_embed.npz from the reference's OWN models (build container only):

    python tests/golden/make_golden_soft_embed.py

sd_30s_soft: the sd_30s waveform (make_golden.py's: synth_audio_batch(1, 480000, 1234)) through the reference SDModel with the
synthetic weights; per encoder frame softmax(logits) @ spk_logit_proj.weight and the row's log-sum-exp, evaluated in float64 from the
reference's fp32 logits -- the per-frame analogue of the soft speaker embeddings below.
asr_soft_embed: the open-set speaker features of tal/asr/gen_embed.py:80-99 from the reference ASRModel('2x', num_speakers=6008) with
speaker ids as vocabulary tokens: a ragged B = 2 batch of synthetic audio (5 s and 4 s), y [2, 25] whose targets carry several speaker
tokens in both rows and one in the padded tail of the second row (y_mask off there: it must be ignored).  Stored: the positions
(nonzero of the speaker mask), the speaker ids (target - vocabulary size) and softmax(logits[:, vocab:]) @ embedding.weight[vocab:] at
those positions, in float64 from the reference's fp32 logits.  The fixtures are data; no reference source is stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden._refload import load_reference  # noqa: E402
from tests.golden.make_golden import _tokens, fill, save  # noqa: E402
from tal_asrd_amd import synth  # noqa: E402

torch.set_grad_enabled(False)
VOCAB, SPEAKERS = 10000, 6008
SEED, LENS = 2025, [80000, 64000]
L, SHORT = 25, 18            # y [2, L]; the second row ends after SHORT tokens
# (row, position in y, speaker): targets are y[:, 1:], so position p of y is target position p - 1
SPEAKER_TOKENS = ((0, 1, 17), (0, 9, 6007), (0, 16, 0), (0, 24, 3001), (1, 3, 4242), (1, 4, 4243), (1, 17, 99), (1, 21, 1234))


def main():
    ns = load_reference()
    # ---- the diarizer head, per frame
    model = fill(ns.models.SDModel())
    audio = torch.from_numpy(synth.synth_audio_batch(1, 480000, 1234))
    enc = model.encode_features(model.extract_features(audio), None)
    logits = model.decode(enc)[0].double()                          # [T', 6008]: the reference's fp32 logits, widened
    table = model.spk_logit_proj.weight.double()
    soft = torch.softmax(logits, dim=-1) @ table
    save("sd_30s_soft", soft=soft.numpy(), lse=torch.logsumexp(logits, dim=-1).numpy(), max_abs_values=float(table.abs().max()),
         audio_seed=1234, audio_len=480000)
    print("sd_30s_soft", tuple(soft.shape), float(soft.abs().max()))

    # ---- the joint model, at the speaker tokens of a transcript
    model = fill(ns.models.ASRModel("2x", num_speakers=SPEAKERS, vocab_size=VOCAB, use_speaker_head=False))
    audio = torch.from_numpy(synth.synth_audio_batch(2, LENS[0], SEED, lens=LENS))
    y = torch.from_numpy(_tokens("soft_embed/y", 2, L, vocab=VOCAB))
    y[1, SHORT:] = 2                                                # (pad)
    for row, pos, spk in SPEAKER_TOKENS:
        y[row, pos] = VOCAB + spk
    y_mask = torch.ones(2, L, dtype=torch.bool)
    y_mask[1, SHORT:] = False
    assert any(row == 1 and pos >= SHORT for row, pos, _ in SPEAKER_TOKENS)
    y_prev, y_target = y[:, :-1], y[:, 1:]
    (lm_logits, _), _ = model.forward(audio, y_prev, torch.tensor(LENS))
    # gen_embed.py:83-99, with the padded tail masked out
    speaker_mask = (y_target >= VOCAB) & y_mask[:, 1:]
    speaker_pos = speaker_mask.nonzero()
    speaker_ids = y_target.masked_select(speaker_mask) - VOCAB
    rows = lm_logits.masked_select(speaker_mask.unsqueeze(-1)).view(-1, lm_logits.size(-1)).double()
    table = model.embedding.weight[VOCAB:].double()
    embeds = torch.softmax(rows[:, VOCAB:], dim=-1) @ table
    assert speaker_pos.shape[0] == len(SPEAKER_TOKENS) - 1 and int((y_target >= VOCAB).sum()) == len(SPEAKER_TOKENS)
    save("asr_soft_embed", y=y.numpy(), y_mask=y_mask.numpy(), audio_seed=SEED, audio_lens=np.asarray(LENS), vocab_size=VOCAB,
         num_speakers=SPEAKERS, positions=speaker_pos.numpy(), speaker_ids=speaker_ids.numpy(), embeds=embeds.numpy(),
         max_abs_values=float(table.abs().max()))
    print("asr_soft_embed", speaker_pos.tolist(), speaker_ids.tolist(), tuple(embeds.shape), float(embeds.abs().max()))


if __name__ == "__main__":
    main()
