"""System.generate(search="device"): the beam search with its loop state on the device (tal_beam_ctx, csrc/beam.hip).

(a) the five recorded calls of tests/test_gpu_flow.py / test_gpu_half_audio.py against the same reference fixtures, same assertions;
(b) the device mode against the host mode on the same build: equal sequences, None where the host gives None, speaker logits
    torch.equal -- B x beam x terminate token x force_output on short clips, and the '1x' / embed_size=0 model variants;
(c) transcribe_batch / transcribe_file with search="device";
(d) a device-mode call changes nothing a following default-mode or generate_unaligned call returns."""
import json
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN, golden, has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]


def dev():
    return torch.device("cuda:0")


def _load(model, weights):
    own = model.state_dict()
    for k, v in weights.items():
        own[k] = torch.from_numpy(np.array(v, copy=True))
    model.load_state_dict(own)
    return model.to(dev())


@pytest.fixture(scope="module")
def asr_model(asr_weights):
    from tal_asrd_amd import ASRModel
    return _load(ASRModel("2x", num_speakers=6008, vocab_size=10000, use_speaker_head=True), asr_weights)


def _fixture_audio(g):
    from tal_asrd_amd import synth
    lens = g["audio_lens"].tolist()
    return torch.from_numpy(synth.synth_audio_batch(2, max(lens), int(g["audio_seed"]), lens=lens)).to(dev()), lens


def _check_seqs(seqs, g):
    for i in range(2):
        want = g["seq_%d" % i]
        if want.size == 0:
            assert seqs[i] is None
        else:
            np.testing.assert_array_equal(seqs[i].numpy(), want)


def _check_spk(spks, g):
    for i in range(2):
        np.testing.assert_array_equal(spks[i].argmax(-1).numpy(), g["spk_argmax_%d" % i])
        np.testing.assert_allclose(spks[i][:, ::200].numpy(), g["spk_sample_%d" % i], atol=2e-3, rtol=0)


# ------------------------------------------------------------------ (a) the reference's recorded calls
def test_fixture_beam1_with_speaker_head(asr_model):
    from tal_asrd_amd.system import System
    g = golden("flow_generate_beam1")
    audio, lens = _fixture_audio(g)
    seqs, spks = System(asr_model, spk_weight=1.0).generate(
        audio, torch.zeros(2, 1, dtype=torch.long, device=dev()), torch.tensor(lens), length=int(g["length"]), beam_size=1,
        terminate_token=1, force_half=False, force_output=True, search="device")
    _check_seqs(seqs, g)
    _check_spk(spks, g)


def test_fixture_beam3_terminates(asr_model):
    from tal_asrd_amd.system import System
    g = golden("flow_generate_beam3")
    audio, lens = _fixture_audio(g)
    seqs, spks = System(asr_model, spk_weight=0.0).generate(
        audio, torch.zeros(2, 1, dtype=torch.long, device=dev()), torch.tensor(lens), length=int(g["length"]), beam_size=3,
        terminate_token=int(g["terminate_token"]), force_half=False, force_output=False, search="device")
    _check_seqs(seqs, g)
    assert spks[0] is None and spks[1] is None


@pytest.mark.parametrize("beam", [1, 3])
def test_fixture_lm_shallow_fusion(asr_model, beam):
    from tal_asrd_amd.system import System
    from tal_asrd_amd.tokenizer import SynthTokenizer
    from tests.golden._lm_standin import StandInLM
    g = golden("flow_generate_lm_beam%d" % beam)
    audio, lens = _fixture_audio(g)
    lm = StandInLM().eval().to(dev())
    sys_ = System(asr_model, spk_weight=1.0 if beam == 1 else 0.0, tokenizer=SynthTokenizer(10000), lm=lm, lm_weight=float(g["lm_weight"]))
    seqs, spks = sys_.generate(audio, torch.zeros(2, 1, dtype=torch.long, device=dev()), torch.tensor(lens), length=int(g["length"]),
                               beam_size=beam, terminate_token=int(g["terminate_token"]), force_half=False, force_output=(beam == 1),
                               search="device")
    _check_seqs(seqs, g)
    if beam == 1:
        for i in range(2):
            np.testing.assert_array_equal(spks[i].argmax(-1).numpy(), g["spk_argmax_%d" % i])
        assert (g["seq_0"] != golden("flow_generate_beam1")["seq_0"]).any()


def test_fixture_force_half_default(asr_model):
    from tal_asrd_amd.system import System
    g = golden("flow_generate_beam1_half")
    audio, lens = _fixture_audio(g)
    seqs, spks = System(asr_model, spk_weight=1.0).generate(
        audio, torch.zeros(2, 1, dtype=torch.long, device=dev()), torch.tensor(lens), length=int(g["length"]), beam_size=1,
        terminate_token=1, force_output=True, search="device")
    _check_seqs(seqs, g)
    _check_spk(spks, g)


# ------------------------------------------------------------------ (b) device mode == host mode on the same build
def _clips(B, seed=77):
    from tal_asrd_amd import synth
    lens = [64000, 48000, 80000][:B]                     # 4 s, 3 s, 5 s
    return torch.from_numpy(synth.synth_audio_batch(B, max(lens), seed, lens=lens)).to(dev()), lens


def _same(a, b):
    (seq_a, spk_a), (seq_b, spk_b) = a, b
    assert len(seq_a) == len(seq_b) and len(spk_a) == len(spk_b)
    for x, y in zip(seq_a, seq_b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and torch.equal(x, y)
    for x, y in zip(spk_a, spk_b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)


def _both(sys_, audio, lens, B, **kw):
    prime = torch.zeros(B, 1, dtype=torch.long, device=dev())
    host = sys_.generate(audio, prime, torch.tensor(lens), **kw)
    device = sys_.generate(audio, prime, torch.tensor(lens), search="device", **kw)
    _same(host, device)
    return host


def _produced_token(sys_, audio, lens, B, beam):
    """A token the search really produces a few steps in (row 0 of the beam-search output without a terminate token): with it
    as terminate token slots finish at different steps, which the fixed token 1 need not do on synthetic weights."""
    seqs, _ = sys_.generate(audio, torch.zeros(B, 1, dtype=torch.long, device=dev()), torch.tensor(lens), length=12, beam_size=beam)
    return int(seqs[0][4])


@pytest.mark.parametrize("beam", [1, 3, 4])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_device_mode_equals_host_mode(asr_model, B, beam):
    from tal_asrd_amd.system import System
    audio, lens = _clips(B)
    sys_ = System(asr_model, spk_weight=1.0 if beam == 1 else 0.0)        # (beams + speaker head raise: see below)
    for term in (None, 1, _produced_token(sys_, audio, lens, B, beam)):
        for force_output in (False, True):
            seqs, spks = _both(sys_, audio, lens, B, length=12, beam_size=beam, terminate_token=term, force_output=force_output)
            if term is None or force_output:
                assert all(s is not None for s in seqs)
                assert all((s is not None) == (beam == 1) for s in spks)


@pytest.mark.parametrize("tag", ["1x_spk", "1x_e0"])
def test_device_mode_equals_host_mode_on_the_model_variants(tag):
    """'1x' (d = 256, head dim 64) and embed_size=0 (no factorised embedding: another LM-head arm), weights as in
    tests/test_gpu_decoder.py::test_model_variants_decode_and_greedy_flow."""
    from tal_asrd_amd import ASRModel, synth
    from tal_asrd_amd.system import System
    kw = {"1x_spk": dict(model_type="1x", num_speakers=6008, vocab_size=10000, use_speaker_head=True),
          "1x_e0": dict(model_type="1x", num_speakers=6008, vocab_size=10000, use_speaker_head=True, embed_size=0)}[tag]
    keys = json.load(open(os.path.join(GOLDEN, "state_dict_keys.json")))["ASRModel_" + tag]
    m = _load(ASRModel(**kw), synth.fill_state_dict({k: tuple(s) for k, s in keys}))
    audio, lens = _clips(2, seed=78)
    _both(System(m, spk_weight=1.0), audio, lens, 2, length=12, beam_size=1, terminate_token=1, force_output=True)
    sys_ = System(m, spk_weight=0.0)
    _both(sys_, audio, lens, 2, length=12, beam_size=3, terminate_token=_produced_token(sys_, audio, lens, 2, 3), force_output=False)


def test_device_mode_raises_where_the_host_mode_raises(asr_model):
    """The reference's own mismatch (beams + speaker head: `speaker_out` is not repeated, system.py:168-171) and an
    out-of-range priming token raise in both modes; more than 512 rows is the device mode's own limit."""
    from tal_asrd_amd._native import NativeError
    from tal_asrd_amd.system import System
    audio, lens = _clips(2)
    prime = torch.zeros(2, 1, dtype=torch.long, device=dev())
    for search in ("host", "device"):
        with pytest.raises(NativeError, match="memory must be"):
            System(asr_model, spk_weight=1.0).generate(audio, prime, torch.tensor(lens), length=4, beam_size=3, search=search)
        with pytest.raises(IndexError):
            System(asr_model).generate(audio, prime + 10 ** 6, torch.tensor(lens), length=4, beam_size=1, search=search)
        with pytest.raises(NativeError):
            System(asr_model).generate(audio, prime, torch.tensor(lens), length=2, beam_size=65, search=search)
    # (the failed calls left nothing behind)
    _both(System(asr_model), audio, lens, 2, length=6, beam_size=3, terminate_token=1)


# ------------------------------------------------------------------ (c) transcription entry points
def test_transcription_with_device_search(asr_model):
    from tal_asrd_amd import synth
    from tal_asrd_amd.system import System
    from tal_asrd_amd.transcribe import transcribe_batch, transcribe_file, window_bounds
    with open(os.path.join(GOLDEN, "flow_transcribe.json")) as f:
        g = json.load(f)
    audio = torch.from_numpy(synth.synth_audio_batch(1, g["audio_len"], g["audio_seed"])[0]).to(dev())
    sys_ = System(asr_model, spk_weight=0.0)

    def text(seq):
        return " ".join(str(int(t)) for t in seq)
    for beam in (1, 2):
        got = transcribe_file(audio, sys_, g["window"], g["stride"], batch_size=g["batch_size"], beam_width=beam, length=g["length"],
                              use_eot=True, eot_token_id=g["eot"], decode=text, force_half=False, search="device")
        assert got == g["beam%d_texts" % beam]
    batch = [audio[s:e] for s, e in window_bounds(audio.numel(), g["window"], g["stride"])][:g["batch_size"]]
    want = transcribe_batch(batch, sys_, beam_width=2, length=g["length"], eot_token_id=g["eot"], force_half=False)
    got = transcribe_batch(batch, sys_, beam_width=2, length=g["length"], eot_token_id=g["eot"], force_half=False, search="device")
    assert len(want) == len(got)
    for x, y in zip(want, got):
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y))


# ------------------------------------------------------------------ (d) no side effects on the other decode paths
def test_device_call_leaves_the_other_paths_alone(asr_model):
    """Both modes share the cached K | V pointer arrays and workspaces: a device-mode call in between changes neither what the
    default mode nor what generate_unaligned returns."""
    from tal_asrd_amd import synth
    from tal_asrd_amd.system import System
    sys_ = System(asr_model)
    audio, lens = _clips(2)
    prime = torch.zeros(2, 1, dtype=torch.long, device=dev())
    L = 160000
    long_audio = torch.from_numpy(synth.synth_audio_batch(1, L, 5)).to(dev())

    def host():
        return sys_.generate(audio, prime, torch.tensor(lens), length=10, beam_size=3)

    def unaligned():
        gen, align = sys_.generate_unaligned(long_audio, torch.ones(1, 1, dtype=torch.long, device=dev()), torch.tensor([L]), max_iters=30)
        return gen.cpu(), [(c.clone(), a.clone()) for c, a in align]
    h0, u0 = host(), unaligned()
    sys_.generate(audio, prime, torch.tensor(lens), length=10, beam_size=3, search="device")
    u1 = unaligned()
    sys_.generate(audio, prime, torch.tensor(lens), length=10, beam_size=4, terminate_token=1, search="device")
    h1 = host()
    _same(h0, h1)
    assert torch.equal(u0[0], u1[0]) and len(u0[1]) == len(u1[1])
    for (c0, a0), (c1, a1) in zip(u0[1], u1[1]):
        assert torch.equal(c0, c1) and torch.equal(a0, a1)
