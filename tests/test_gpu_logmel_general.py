"""The general log-mel front-end (csrc/logmel_general.hip) on the GPU: LogMelSpec(sr, n_mels) over a grid of sample rates, mel
counts, batch sizes and lengths against the float64 and fp32 restatements of tests/_logmel_general_ref.py; custom checkpoint
buffers; silence; fp16 waveforms; the `logmel_general` option on the default shape; SDModel / ASRModel(n_mels=...) end to end;
the split-batch (sum, count) contract; call-after-call bit identity; one hour of 48 kHz audio (64-bit offsets)."""
import numpy as np
import pytest
import torch

from tests.conftest import has_gpu
from tests import _logmel_general_ref as G

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

F64_TOL = 5e-5        # from the float64 restatement, before the mean, every frame
MEL_TOL = 1e-3        # from the fp32 torch.stft restatement (the reference's own arithmetic)
MEAN_TOL = 1e-5
LOGIT_TOL = 1e-3

GRID = [(16000, 40), (16000, 64), (16000, 128), (8000, 40), (8000, 128), (22050, 80), (44100, 128), (48000, 16), (16000, 23)]


def dev():
    return torch.device("cuda:0")


def _audio(B, L, seed):
    from tal_asrd_amd import synth
    return synth.synth_audio_batch(B, L, seed)


def _module(sr, n_mels):
    from tal_asrd_amd import LogMelSpec
    return LogMelSpec(sr=sr, n_mels=n_mels).to(dev())


def _bufs(m):
    t = m.mel_transform
    return t.spectrogram.window.cpu(), t.mel_scale.fb.cpu(), t.hop_length


def _run(m, audio):
    from tal_asrd_amd import ops
    x = torch.from_numpy(audio).to(dev())
    out, mean, stats = ops.logmel(m.plan(), x, eps=m.eps, subtract_mean=False, return_stats=True)
    sub = m(x)
    torch.cuda.synchronize()
    return out.cpu().numpy(), float(mean.cpu()), stats.cpu().numpy(), sub.cpu().numpy()


@pytest.mark.parametrize("sr,n_mels", GRID)
@pytest.mark.parametrize("B", [1, 3])
def test_grid_against_float64_and_fp32(sr, n_mels, B):
    m = _module(sr, n_mels)
    win, fb, hop = _bufs(m)
    n_fft = win.shape[0]
    assert (n_fft, hop) == G.shape_for(sr)
    for L in (n_fft // 2 + 1, 37 * hop, sr, 60 * sr):
        audio = _audio(B, L, 7 + L % 1000 + B)
        out, mean, stats, sub = _run(m, audio)
        T = 1 + (L + 2 * (n_fft // 2) - n_fft) // hop          # torch.stft's count (odd n_fft: one less when hop | L)
        assert out.shape == (B, T, n_mels)
        ref64 = G.logmel_f64(audio, win.double().numpy(), fb.double().numpy(), hop, subtract_mean=False)
        err64 = np.abs(out - ref64).max()
        assert err64 <= F64_TOL, (sr, n_mels, B, L, err64)
        ref32 = G.logmel_f32(audio, win, fb, hop, subtract_mean=False).numpy()
        assert np.abs(out - ref32).max() <= MEL_TOL, (sr, n_mels, B, L)
        assert stats[1] == B * T * n_mels
        assert abs(stats[0] / stats[1] - ref64.mean()) <= MEAN_TOL
        assert abs(mean - ref64.mean()) <= MEAN_TOL
        assert np.abs(sub - (ref64 - ref64.mean())).max() <= F64_TOL + MEAN_TOL


def test_custom_window_and_filterbank_buffers():
    """A non-Hann window and a random non-negative filterbank, loaded as checkpoint buffers, against float64."""
    m = _module(22050, 48)
    n_fft = m.mel_transform.spectrogram.window.shape[0]
    g = torch.Generator().manual_seed(5)
    win = (0.54 - 0.46 * torch.cos(2 * np.pi * torch.arange(n_fft, dtype=torch.float64) / (n_fft - 1))).float()
    win = win * (1 + 0.01 * torch.rand(n_fft, generator=g))            # asymmetric on purpose
    fb = torch.rand(n_fft // 2 + 1, 48, generator=g) * (torch.rand(n_fft // 2 + 1, 48, generator=g) < 0.3)
    sd = m.state_dict()
    sd["mel_transform.spectrogram.window"] = win
    sd["mel_transform.mel_scale.fb"] = fb
    m.load_state_dict(sd)
    audio = _audio(2, 3 * 22050 + 17, 99)
    out, _, _, _ = _run(m, audio)
    ref64 = G.logmel_f64(audio, win.double().numpy(), fb.double().numpy(), m.mel_transform.hop_length, subtract_mean=False)
    assert np.abs(out - ref64).max() <= F64_TOL


def test_silence_gives_log_eps_and_zero_after_the_mean():
    from tal_asrd_amd import ops
    m = _module(8000, 128)               # 8 kHz / 128 mels: filters with empty support too
    B, L = 3, 8000 * 2 + 5
    x = torch.zeros(B, L, device=dev())
    out, mean, stats = ops.logmel(m.plan(), x, eps=m.eps, subtract_mean=False, return_stats=True)
    sub = m(x)
    T = 1 + L // 80
    # the kernel's logf(0 + eps), against the device's own float32 log of eps: every output, every bit
    log_eps = torch.log(torch.full((1,), m.eps, dtype=torch.float32, device=dev()))
    assert torch.equal(out, log_eps.expand_as(out))
    assert abs(float(log_eps) - float(np.log(np.float32(m.eps)))) <= 1e-6        # (and it is the log of eps)
    assert torch.all(sub == 0).item()
    assert float(stats[1].cpu()) == B * T * 128


@pytest.mark.parametrize("sr,n_mels,L", [(16000, 40, 480000), (48000, 128, 48000 * 7 + 3), (8000, 23, 1001)])
def test_half_waveform_equals_widened_fp32_bit_for_bit(sr, n_mels, L):
    m = _module(sr, n_mels)
    a32 = torch.from_numpy(_audio(2, L, 3)).to(dev())
    a16 = a32.half()
    with torch.no_grad():
        h = m(a16)
        f = m(a16.float())
    assert torch.equal(h, f)


def test_option_forces_the_general_kernel_on_the_default_shape():
    from oracle import tal_oracle as O
    from tal_asrd_amd import _native as N, ops
    m = _module(16000, 80)
    win, fb = m.mel_transform.spectrogram.window, m.mel_transform.mel_scale.fb
    audio = _audio(2, 16000 * 20 + 77, 21)
    x = torch.from_numpy(audio).to(dev())
    before = ops.logmel(ops.logmel_plan(win, fb), x, subtract_mean=False).cpu().numpy()
    N.set_option("logmel_general", 1)
    try:
        plan = ops.logmel_plan(win, fb)
        assert isinstance(plan, ops.LogmelGeneralPlan)
        gen = ops.logmel(plan, x, subtract_mean=False).cpu().numpy()
    finally:
        N.set_option("logmel_general", 0)
    after = ops.logmel(ops.logmel_plan(win, fb), x, subtract_mean=False).cpu().numpy()
    assert not isinstance(ops.logmel_plan(win, fb), ops.LogmelGeneralPlan)
    np.testing.assert_array_equal(after, before)
    ref64 = G.logmel_f64(audio, win.cpu().double().numpy(), fb.cpu().double().numpy(), 160, subtract_mean=False)
    assert np.abs(gen - ref64).max() <= F64_TOL
    assert np.abs(gen - before).max() <= F64_TOL
    assert np.abs(gen - O.logmel(audio, subtract_mean=False).numpy()).max() <= MEL_TOL


def _load(model, seed=0):
    from tal_asrd_amd import synth
    own = model.state_dict()
    shapes = {k: tuple(v.shape) for k, v in own.items() if "mel_transform" not in k}
    for k, v in synth.fill_state_dict(shapes).items():
        own[k] = torch.from_numpy(np.array(v, copy=True))
    model.load_state_dict(own)
    return model.to(dev())


@pytest.mark.parametrize("n_mels", [40, 64])
def test_sd_model_end_to_end(n_mels):
    """SDModel(n_mels): the log-mel stage against float64, speaker_ids (premean path) against decode(encode(...)).argmax,
    fp16 audio equal to its widened copy."""
    from tal_asrd_amd import SDModel
    m = _load(SDModel(n_mels=n_mels))
    audio = _audio(1, 16000 * 30, 1234)
    x = torch.from_numpy(audio).to(dev())
    with torch.no_grad():
        mel = m.extract_features(x)
        enc = m.encode_features(mel)
        logits = m.decode(enc)
        feat, ids, ids_logits = m.speaker_ids(x, want_logits=True)
        e16 = m.encode(x.half())["encoder_out"]
        e32 = m.encode(x.half().float())["encoder_out"]
    torch.cuda.synchronize()
    win, fb, hop = _bufs(m.logmelspec)
    ref = G.logmel_f64(audio, win.double().numpy(), fb.double().numpy(), hop)
    assert np.abs(mel.cpu().numpy() - ref).max() <= F64_TOL + MEAN_TOL
    assert enc["encoder_out"].shape[-1] == 18 * n_mels and torch.isfinite(logits).all()
    assert np.abs(ids_logits.cpu().numpy().reshape(logits.shape) - logits.cpu().numpy()).max() <= LOGIT_TOL
    lg = logits.reshape(-1, logits.shape[-1])
    top2 = torch.topk(lg, 2, dim=-1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-3
    assert torch.equal(ids.reshape(-1).long()[clear], lg.argmax(-1)[clear])
    assert torch.equal(e16, e32)


@pytest.mark.parametrize("name,n_mels", [("sd_n40_30s", 40), ("sd_n64_30s", 64)])
def test_sd_model_golden_from_the_reference(name, n_mels):
    """SDModel(n_mels) against the reference's own SDModel(n_mels) (tests/golden/make_golden_mel_variants.py): log-mel rows
    (MEL_TOL), encoder rows and channel sums, logits (1e-3), embeddings, IDENTICAL speaker ids; then the fused speaker_ids path
    (the mean folded into the first resize conv) gives the same ids.  40 mels: 400 / 560 / 720 channels in 40 groups; 64 mels:
    640 / 896 / 1152 channels in 64 groups -- other kernel families than the 80-mel model's."""
    from tests.conftest import golden
    from tests.test_gpu_parity import _check_sd_golden
    from tal_asrd_amd import SDModel, synth
    m = _load(SDModel(n_mels=n_mels))
    err = _check_sd_golden(m, name, False)
    print("%s max logit err %.3e" % (name, err))
    g = golden(name)
    audio = torch.from_numpy(synth.synth_audio_batch(1, int(g["audio_len"]), int(g["audio_seed"]))).to(dev())
    with torch.no_grad():
        _, ids = m.speaker_ids(audio)
    np.testing.assert_array_equal(ids.reshape(-1).cpu().numpy(), g["ids"].reshape(-1))


def test_asr_model_n40_golden_from_the_reference():
    """ASRModel('2x', n_mels=40, num_speakers=6008, use_speaker_head=True).encode on the ragged B = 2 call against the
    reference's (asr_n40_enc_b2): encoder_out / speaker_out rows within 1e-3, channel sums, padding mask identical."""
    from tests.conftest import golden
    from tal_asrd_amd import ASRModel, synth
    m = _load(ASRModel("2x", n_mels=40, num_speakers=6008, use_speaker_head=True))
    g = golden("asr_n40_enc_b2")
    lens = g["audio_lens"].tolist()
    audio = torch.from_numpy(synth.synth_audio_batch(2, 480000, int(g["audio_seed"]), lens=lens)).to(dev())
    with torch.no_grad():
        enc = m.encode(audio, torch.tensor(lens))
    r = g["rows"]
    np.testing.assert_allclose(enc["encoder_out"][:, r].cpu().numpy(), g["encoder_out"], atol=LOGIT_TOL, rtol=0)
    np.testing.assert_allclose(enc["speaker_out"][:, r].cpu().numpy(), g["speaker_out"], atol=LOGIT_TOL, rtol=0)
    np.testing.assert_allclose(enc["encoder_out"].double().sum(dim=1).cpu().numpy(), g["enc_sum"], atol=5e-2, rtol=1e-4)
    np.testing.assert_allclose(enc["speaker_out"].double().sum(dim=1).cpu().numpy(), g["spk_sum"], atol=5e-2, rtol=1e-4)
    np.testing.assert_array_equal(enc["encoder_padding_mask"].cpu().numpy(), g["mask"])


def test_split_batch_stats_equal_the_one_call_result():
    """B = 4 at 40 mels as 2 + 2 with the combined (sum, count) == the one-call result."""
    from tal_asrd_amd import ops
    m = _module(16000, 40)
    x = torch.from_numpy(_audio(4, 16000 * 15 + 9, 41)).to(dev())
    one = m(x)
    a, _, sa = ops.logmel(m.plan(), x[:2], subtract_mean=False, return_stats=True)
    b, _, sb = ops.logmel(m.plan(), x[2:], subtract_mean=False, return_stats=True)
    mean = (sa[0] + sb[0]) / (sa[1] + sb[1])
    two = torch.cat([a, b]) - mean.float()
    assert float((one - two).abs().max()) <= 1e-6


@pytest.mark.parametrize("sr,n_mels", [(16000, 40), (48000, 128)])
def test_call_after_call_bit_identity(sr, n_mels):
    m = _module(sr, n_mels)
    x = torch.from_numpy(_audio(1, sr * 300, 8)).to(dev())
    r0 = m(x)
    for _ in range(2):
        assert torch.equal(m(x), r0)


def test_one_hour_at_48khz_128_mels():
    from tal_asrd_amd import ops
    m = _module(48000, 128)
    win, fb, hop = _bufs(m)
    L = 48000 * 3600
    g = torch.Generator(device=dev()).manual_seed(3)
    x = (torch.rand(1, L, generator=g, device=dev()) - 0.5) * 0.6
    out = ops.logmel(m.plan(), x, subtract_mean=False)
    T = 1 + L // hop
    assert out.shape == (1, T, 128)
    host = x[0].cpu().numpy()
    for f0 in (0, T // 2 - 20, T - 40):
        ref = G.logmel_f64_frames(host, win.double().numpy(), fb.double().numpy(), hop, f0, f0 + 40)
        got = out[0, f0:f0 + 40].cpu().numpy()
        assert np.abs(got - ref).max() <= F64_TOL, f0
