"""Pin the float64 decoder reference (tests/_decoder_ref.py) that tests/test_gpu_decoder_kernels.py measures the kernels
against: it must reproduce the fixtures recorded from the reference's own modules within the tolerances of their GPU tests
(tests/test_gpu_decoder.py), and agree with the CPU oracle when run in float32.  CPU only."""
import numpy as np
import pytest
import torch

from oracle import tal_oracle as O
from tal_asrd_amd import synth
from tests import _decoder_ref as R
from tests.conftest import golden

LOGIT_TOL = 1e-3      # tests/test_gpu_decoder.py
ATTN_TOL = 1e-4
LAYER_TOL = 2e-5      # test_decoder_layer_small_golden
ORACLE_TOL = 2e-5     # two float32 restatements of the same arithmetic (tests/test_oracle_golden.py)


def _layer_shapes(E, FF):
    sh = {"resweight": (1,), "resweight_src": (1,)}
    for a in ("self_attn", "multihead_attn"):
        sh[a + ".in_proj_weight"] = (3 * E, E)
        sh[a + ".in_proj_bias"] = (3 * E,)
        sh[a + ".out_proj.weight"] = (E, E)
        sh[a + ".out_proj.bias"] = (E,)
    sh.update({"linear1.weight": (FF, E), "linear1.bias": (FF,), "linear2.weight": (E, FF), "linear2.bias": (E,)})
    return sh


def _declayer_sd():
    sd = synth.fill_state_dict({"declayer." + k: s for k, s in _layer_shapes(64, 256).items()})
    return {k[len("declayer."):]: v for k, v in sd.items()}


def _mask_cases(U, kpm):
    cm = R.causal_mask(U)
    return (("plain", None, None), ("causal", cm, None), ("kpm", None, kpm), ("causal_kpm", cm, kpm))


def test_decoder_layer_small_golden_float64():
    g = golden("declayer_small")
    sd = _declayer_sd()
    tgt, mem = g["tgt"].transpose(1, 0, 2), g["mem"].transpose(1, 0, 2)      # [U,B,E] -> [B,U,E]
    for tag, tm, km in _mask_cases(7, g["kpm"]):
        y, w, _ = R.decoder_layer(tgt, mem, sd, 4, tgt_mask=tm, kpm=km)
        np.testing.assert_allclose(y.numpy().transpose(1, 0, 2), g["y_" + tag], atol=LAYER_TOL, rtol=0, err_msg=tag)
        np.testing.assert_allclose(w.numpy(), g["w_" + tag], atol=ATTN_TOL, rtol=0, err_msg=tag)


def _realistic_layer(E, FF, seed):
    g = torch.Generator().manual_seed(seed)
    p = {}
    for k, s in _layer_shapes(E, FF).items():
        if k.startswith("resweight"):
            p[k] = 0.3 + 0.7 * torch.rand(s, generator=g)
        elif k.endswith("bias"):
            p[k] = 0.1 * torch.randn(s, generator=g)
        else:
            p[k] = torch.randn(s, generator=g) / s[1] ** 0.5
    return p


@pytest.mark.parametrize("saturated", [True, False])
def test_decoder_layer_float32_matches_oracle(saturated):
    """The reference in float32 and the oracle (oracle/tal_oracle.py: [U,B,E], its own mha) compute the same numbers, on the
    synthetic weights of the fixtures and at a realistic weight scale (attention spread over many keys)."""
    B, U, S, E, H = 2, 9, 37, 64, 4
    sd = _declayer_sd() if saturated else {k: v.numpy() for k, v in _realistic_layer(E, 256, 5).items()}
    g = torch.Generator().manual_seed(11)
    tgt, mem = torch.randn(B, U, E, generator=g), torch.randn(B, S, E, generator=g)
    kpm = torch.zeros(B, S, dtype=torch.bool)
    kpm[1, 30:] = True
    kpm[0, 3:5] = True
    for tag, tm, km in _mask_cases(U, kpm):
        want, ww = O.decoder_layer(tgt.permute(1, 0, 2), mem.permute(1, 0, 2), sd, "", H,
                                   tgt_mask=None if tm is None else tm.float(), memory_key_padding_mask=km)
        y, w, probs = R.decoder_layer(tgt, mem, sd, H, tgt_mask=tm, kpm=km, dtype=torch.float32)
        np.testing.assert_allclose(y.numpy(), want.permute(1, 0, 2).numpy(), atol=ORACLE_TOL, rtol=0, err_msg=tag)
        np.testing.assert_allclose(w.numpy(), ww.numpy(), atol=ORACLE_TOL, rtol=0, err_msg=tag)
        if km is not None:
            assert float(probs[1, :, :, 30:].abs().max()) == 0.0


@pytest.fixture(scope="module")
def oracle_memory():
    """The window the recorded decode fixtures were made on, encoded by the CPU oracle (as tests/test_oracle_golden.py does)."""
    from tests.conftest import GOLDEN
    import json
    import os
    keys = json.load(open(os.path.join(GOLDEN, "state_dict_keys.json")))["ASRModel_2x_spk"]
    sd = synth.fill_state_dict({k: tuple(s) for k, s in keys})
    S = int(golden("asr_decode")["S"])
    with torch.no_grad():
        enc = O.asr_encode(synth.synth_audio_batch(1, 480000, 1234), sd, [480000])
    return sd, enc["encoder_out"][:, :S].contiguous(), enc["encoder_padding_mask"][:, :S]


def _stack(sd, prefix, n):
    return [{k[len(prefix) + len("%d." % l):]: v for k, v in sd.items() if k.startswith("%s%d." % (prefix, l))}
            for l in range(n)]


def test_asr_decode_golden_float64(oracle_memory):
    """ASRModel.decode of the '2x' model: first and last logits rows and every layer's last attention row."""
    sd, mem, mask = oracle_memory
    g = golden("asr_decode")
    layers = _stack(sd, "decoder.layers.", 4)
    pe = R.positional_encoding(512, 512)
    for U in (1, 7, 64):
        y = g["y_%d" % U]
        x = R.embed_tokens(y, sd["embedding.weight"], sd["embedding_proj.weight"], pe)
        for causal in (True, False):
            tag = "U%d_%s" % (U, "causal" if causal else "full")
            h, avgs = R.decoder_stack(x, mem, layers, 4, tgt_mask=R.causal_mask(U) if causal else None, kpm=mask)
            logits = R.lm_logits(h, sd["embedding.weight"], sd["embedding_proj.weight"]).numpy()
            np.testing.assert_allclose(logits[:, -1], g["logits_last_" + tag], atol=LOGIT_TOL, rtol=0, err_msg=tag)
            np.testing.assert_allclose(logits[:, 0], g["logits_first_" + tag], atol=LOGIT_TOL, rtol=0, err_msg=tag)
            attn = np.stack([a[:, -1].numpy() for a in avgs], 0)
            np.testing.assert_allclose(attn, g["attn_last_" + tag], atol=ATTN_TOL, rtol=0, err_msg=tag)
            assert R.greedy_pick(logits[0, -1]) == int(np.argmax(g["logits_last_" + tag][0]))
            if not causal:
                # the greedy step's form: the last row of a causal-free decode, its attention averaged over layers
                scores, row = R.greedy_step(y[0], mem[0], mask[0], layers, 4, sd["embedding.weight"],
                                            sd["embedding_proj.weight"], pe)
                np.testing.assert_allclose(scores.numpy(), logits[0, -1], atol=1e-9, rtol=0)
                np.testing.assert_allclose(row.numpy(), attn[:, 0].mean(0), atol=1e-12, rtol=0)


def test_asr_decode_float32_matches_oracle(oracle_memory):
    sd, mem, mask = oracle_memory
    g = golden("asr_decode")
    layers = _stack(sd, "decoder.layers.", 4)
    y = g["y_7"]
    with torch.no_grad():
        want, wattn = O.asr_decode(y, {"encoder_out": mem, "encoder_padding_mask": mask}, sd, causal_mask=True)
    x = R.embed_tokens(y, sd["embedding.weight"], sd["embedding_proj.weight"], R.positional_encoding(512, 512, torch.float32),
                       torch.float32)
    h, avgs = R.decoder_stack(x, mem, layers, 4, tgt_mask=R.causal_mask(7, torch.float32), kpm=mask, dtype=torch.float32)
    logits = R.lm_logits(h, sd["embedding.weight"], sd["embedding_proj.weight"], torch.float32)
    np.testing.assert_allclose(logits.numpy(), want.numpy(), atol=LOGIT_TOL, rtol=0)
    for a, b in zip(avgs, wattn):
        np.testing.assert_allclose(a.numpy(), b.numpy(), atol=ATTN_TOL, rtol=0)


def test_beam_topk_reference_is_stable():
    lp = np.array([[[0.0, -1.0, 0.0], [0.0, -2.0, -1.0]]])
    vals, ids = R.beam_topk(lp, np.zeros((1, 2)), None, 4)
    np.testing.assert_array_equal(ids, [[0, 2, 3, 1]])
    vals, ids = R.beam_topk(lp, None, np.ones((1, 2), dtype=bool), 3)
    np.testing.assert_array_equal(ids, [[0, 1, 2]])
    assert np.all(np.isneginf(vals))
    assert R.greedy_pick([1.0, 3.0, 3.0]) == 1
