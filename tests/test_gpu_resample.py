"""The device resampler (csrc/resample.hip, tal_asrd_amd.Resample, the models' sample_rate= argument) against the float64
restatement of tests/_resample_ref.py.

Tolerance: _resample_ref.err_bound, the a-priori bound of an fp32 FMA chain over fp32-rounded weights,
(taps + 2) 2^-24 max_p sum_j |w[p][j]| max|x| -- derived, not tuned.  Everything that promises identity (exact widening of
int16 / fp16, batch position, ragged rows, call after call) is compared bit for bit.
"""
import contextlib
import threading

import numpy as np
import pytest
import torch

from tests import _resample_ref as R
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

LOGIT_TOL = 1e-3      # BASELINE.json north_star: logits within 1e-3 fp32

PAIRS = [(44100, 16000), (48000, 16000), (8000, 16000), (22050, 16000), (11025, 16000), (32000, 16000), (16000, 8000),
         (16000, 16000), (16000, 44100),
         (16001, 16000)]          # 16000 phases: the table is read through L2 instead of sitting in LDS


def dev():
    return torch.device("cuda:0")


def _lengths(orig, new):
    iu, _, taps, _, _ = R.plan_f64(orig, new)
    return [1, taps - 1, iu, iu + 1, 3 * iu, 4097, orig // 2 + 37, 5 * orig]      # 3 iu: an exact multiple; 5 s: many workgroups


@pytest.fixture(scope="module")
def waves():
    """One uniform(-1, 1) float32 pool [3, 5 * 48000 + 64]; every case takes a prefix of it (unchanged by the tests)."""
    x = np.random.default_rng(20240).uniform(-1.0, 1.0, size=(3, 5 * 48000 + 64)).astype(np.float32)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("orig,new", PAIRS)
def test_grid_against_float64(waves, orig, new, B):
    from tal_asrd_amd import Resample
    rs = Resample(orig, new)
    worst = 0.0
    for L in _lengths(orig, new):
        x = np.array(waves[:B, :L])
        xd = torch.from_numpy(x).to(dev())
        y = rs(xd)
        want = R.resample_f64(x, orig, new)
        assert tuple(y.shape) == (B, R.num_samples(L, orig, new)) == want.shape and y.dtype == torch.float32
        bound = R.err_bound(x, orig, new)
        err = float(np.abs(y.cpu().numpy().astype(np.float64) - want).max())
        yt = R.resample_torch(xd, orig, new)
        assert yt.shape == y.shape
        err_t = float((y - yt).abs().max())
        worst = max(worst, err / bound)
        print("%d -> %d B=%d L=%d: |err| %.3e, vs conv1d %.3e, bound %.3e" % (orig, new, B, L, err, err_t, bound))
        assert err <= bound, (L, err, bound)
        assert err_t <= 2 * bound, (L, err_t, bound)
    print("%d -> %d B=%d: worst error / bound = %.3f" % (orig, new, B, worst))


@pytest.mark.parametrize("orig,new", [(44100, 16000), (8000, 16000), (16001, 16000)])
def test_exact_widening(orig, new):
    """int16 input == the fp32 call on x * 2^-15, fp16 input == the fp32 call on the widened samples, bit for bit, with the 16-bit
    data starting at odd element offsets of a larger buffer (2-byte-aligned starts of the 16-byte loads)."""
    from tal_asrd_amd import Resample
    rs = Resample(orig, new)
    rng = np.random.default_rng(5)
    L = 3 * 4096 + 77
    pcm = torch.from_numpy(rng.integers(-32768, 32768, size=L + 16, dtype=np.int16)).to(dev())
    pcm[3], pcm[4] = -32768, 32767
    half = torch.from_numpy(rng.uniform(-1, 1, size=L + 16).astype(np.float16)).to(dev())
    for off in (1, 3, 8):
        a = pcm[off:off + L]
        assert a.data_ptr() % 16 == (pcm.data_ptr() + 2 * off) % 16
        want = rs((a.to(torch.float32) * 2.0 ** -15).unsqueeze(0))
        assert torch.equal(rs(a.unsqueeze(0)), want) and torch.equal(rs(a), want[0])
        h = half[off:off + L]
        assert torch.equal(rs(h.unsqueeze(0)), rs(h.to(torch.float32).unsqueeze(0)))
    f = torch.from_numpy(rng.uniform(-1, 1, size=L + 16).astype(np.float32)).to(dev())
    assert torch.equal(rs(f[1:1 + L]), rs(f[1:1 + L].clone()))            # fp32 at a 4-byte-aligned, not 16-byte-aligned start


@pytest.mark.parametrize("orig,new", [(44100, 16000), (8000, 16000), (16001, 16000)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
def test_ragged_batch(orig, new, dtype):
    """[3, L] with lengths (L, L // 2 + 5, 1): row b equals the B = 1 call on x[b, :len_b] bit for bit up to n_out(len_b) and is
    exactly zero beyond; without lengths, a row in the batch equals the same row alone (the tiling differs: tiles are dealt to
    workgroups over the whole batch)."""
    from tal_asrd_amd import Resample
    rs = Resample(orig, new)
    L = 2 * 4096 + 301
    rng = np.random.default_rng(11)
    if dtype == torch.int16:
        x = torch.from_numpy(rng.integers(-32768, 32768, size=(3, L), dtype=np.int16)).to(dev())
    else:
        x = torch.from_numpy(rng.uniform(-1, 1, size=(3, L)).astype(np.float32)).to(dev())
    lens = [L, L // 2 + 5, 1]
    y = rs(x, lengths=torch.tensor(lens))
    whole = rs(x)
    assert y.shape == whole.shape == (3, R.num_samples(L, orig, new))
    for b, lb in enumerate(lens):
        nb = R.num_samples(lb, orig, new)
        alone = rs(x[b, :lb].clone().unsqueeze(0))
        assert alone.shape == (1, nb)
        assert torch.equal(y[b, :nb], alone[0]), b
        assert int((y[b, nb:] != 0).sum()) == 0, b
        assert torch.equal(whole[b], rs(x[b:b + 1].clone())[0]), b
    xn = x.cpu().numpy()
    want = R.resample_f64(xn, orig, new, lengths=lens)
    assert float(np.abs(y.cpu().numpy() - want).max()) <= R.err_bound(xn, orig, new)


@contextlib.contextmanager
def hog(active):
    """While the block runs, a host thread keeps 256 MB device-to-device copies in flight on a stream of its own."""
    if not active:
        yield
        return
    d = dev()
    stream = torch.cuda.Stream(device=d)
    with torch.cuda.stream(stream):
        a = torch.empty(64 * 1024 * 1024, dtype=torch.float32, device=d).normal_()
        b = torch.empty_like(a)
    stream.synchronize()
    stop = threading.Event()
    copies = [0]

    def run():
        pending = []
        with torch.cuda.device(d), torch.cuda.stream(stream):
            while not stop.is_set():
                b.copy_(a, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(stream)
                pending.append(ev)
                copies[0] += 1
                if len(pending) >= 3:
                    pending.pop(0).synchronize()
        stream.synchronize()

    t = threading.Thread(target=run, daemon=True)
    t.start()
    try:
        yield
    finally:
        stop.set()
        t.join()
        assert copies[0] >= 3, "the bandwidth hog never ran beside the test"


@pytest.mark.parametrize("contended", [pytest.param(False, id="quiet"), pytest.param(True, id="bandwidth-hog")])
def test_the_same_call_after_call(contended):
    """5 minutes of 44.1 kHz PCM (B = 2) and 30 s through the L2 form: every call's output equals the first call's bit for bit,
    quiet and with a second stream pulling on the memory system."""
    from tal_asrd_amd import Resample
    rng = np.random.default_rng(3)
    cases = [(Resample(44100, 16000), torch.from_numpy(rng.integers(-32768, 32768, size=(2, 300 * 44100), dtype=np.int16)).to(dev())),
             (Resample(16001, 16000), torch.from_numpy(rng.uniform(-1, 1, size=(1, 30 * 16001)).astype(np.float32)).to(dev()))]
    for rs, x in cases:
        y0 = rs(x).clone()
        bad = 0
        with hog(contended):
            for _ in range(40):
                bad += int(not torch.equal(rs(x), y0))
        assert bad == 0, "%d -> %d: %d of 40 calls differ from the first" % (rs.orig_freq, rs.new_freq, bad)


def test_offsets_beyond_2_31():
    """B = 2 items of 2^30 + 12345 int16 samples, 44100 -> 16000: the last element index is above 2^31 on both sides of the copy
    (4.3 GB in, 3.1 GB out).  The input is filled on the device; 4096-sample windows at the start, on either side of the item
    boundary and at the end are compared with the float64 definition on the matching input slices."""
    free, _ = torch.cuda.mem_get_info(dev())
    if free < 12 * 2 ** 30:
        pytest.skip("needs 12 GB of free device memory, %.1f GB are free" % (free / 2 ** 30))
    from tal_asrd_amd import Resample
    orig, new = 44100, 16000
    L = 2 ** 30 + 12345
    rs = Resample(orig, new)
    x = torch.empty(2, L, dtype=torch.int16, device=dev())
    # a cheap device-side fill with no short period: a wrapped multiplicative ramp, item 1 offset from item 0
    for c in range(0, L, 2 ** 26):
        idx = torch.arange(c, min(c + 2 ** 26, L), dtype=torch.int64, device=dev())
        x[0, c:c + 2 ** 26] = ((idx * 7919) & 0xffff).to(torch.int16)
        x[1, c:c + 2 ** 26] = ((idx * 104729 + 12345) & 0xffff).to(torch.int16)
    del idx
    y = rs(x)
    n = R.num_samples(L, orig, new)
    assert tuple(y.shape) == (2, n)
    assert 2 * L > 2 ** 31 and 2 * n * 4 > 2 ** 31      # input element indices and output byte offsets beyond 2^31
    iu, ou, taps, first, _ = R.plan_f64(orig, new)
    W = 4096
    worst = 0.0
    for b, m0 in ((0, 0), (0, n - W), (1, 0), (1, n - W)):
        lo = max(0, (m0 // ou) * iu + int(first.min()) - 8)
        hi = min(L, ((m0 + W) // ou + 1) * iu + int(first.max()) + taps + 8)
        xs = x[b, lo:hi].cpu().numpy()
        want = R.window_f64(xs, lo, L, orig, new, m0, W)
        got = y[b, m0:m0 + W].cpu().numpy().astype(np.float64)
        bound = R.err_bound(xs, orig, new)
        err = float(np.abs(got - want).max())
        print("item %d outputs %d..: |err| %.3e bound %.3e" % (b, m0, err, bound))
        worst = max(worst, err / bound)
        assert err <= bound, (b, m0, err, bound)
        assert float(np.abs(want).max()) > 1e-3
    del x, y
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- end to end
def _load(model, sd):
    own = model.state_dict()
    for k, v in sd.items():
        own[k] = torch.from_numpy(np.array(v, copy=True))
    model.load_state_dict(own)
    return model.to(dev()).eval()


@pytest.fixture(scope="module")
def sd_model(sd_weights):
    from tal_asrd_amd import SDModel
    return _load(SDModel(), sd_weights)


@pytest.fixture(scope="module")
def asr_model(asr_weights):
    from tal_asrd_amd import ASRModel
    return _load(ASRModel("2x", num_speakers=6008, vocab_size=10000, use_speaker_head=True), asr_weights)


def _pcm(seconds, rate, seed):
    """Synthetic speech-like audio at `rate` as 16-bit PCM [1, L] (host)."""
    from tal_asrd_amd import synth
    a = synth.synth_audio_batch(1, int(seconds * rate), seed)
    return torch.from_numpy(np.round(a * 32767.0).astype(np.int16))


def test_speaker_ids_from_pcm(sd_model):
    """SDModel.speaker_ids(pcm16 at 44.1 kHz, sample_rate=44100) == speaker_ids(Resample(44100, 16000)(pcm16))."""
    from tal_asrd_amd import Resample
    x = _pcm(20, 44100, 7).to(dev())
    with torch.no_grad():
        feat, ids, logits = sd_model.speaker_ids(x, want_logits=True, sample_rate=44100)
        f2, i2, l2 = sd_model.speaker_ids(Resample(44100, 16000)(x), want_logits=True)
    assert torch.equal(ids, i2)
    assert float((logits - l2).abs().max()) <= LOGIT_TOL and float((feat - f2).abs().max()) <= LOGIT_TOL
    assert ids.numel() > 200


def test_speaker_ids_stream_from_pcm(sd_model):
    clips = [_pcm(sec, 44100, seed) for sec, seed in ((12, 1), (20, 2), (7, 3))]
    with torch.no_grad():
        got = list(sd_model.speaker_ids_stream(clips, sample_rate=44100))
        assert len(got) == 3
        for clip, (feat, ids) in zip(clips, got):
            f2, i2 = sd_model.speaker_ids(clip.to(dev()), sample_rate=44100)
            assert torch.equal(ids, i2) and torch.equal(feat, f2)


def test_asr_encode_at_8_khz(asr_model):
    """ASRModel.encode(x, audio_lens, sample_rate=8000) == encode of the resampled batch with audio_lens mapped through n_out."""
    from tal_asrd_amd import Resample, synth
    lens = [80000, 66001]
    x = torch.from_numpy(synth.synth_audio_batch(2, 80000, 5, lens=lens)).to(dev())
    al = torch.tensor(lens)
    rs = Resample(8000, 16000)
    with torch.no_grad():
        a = asr_model.encode(x, al, sample_rate=8000)
        mapped = rs.num_samples(al)
        assert mapped.tolist() == [R.num_samples(l, 8000, 16000) for l in lens]
        b = asr_model.encode(rs(x, lengths=al), mapped)
        c = asr_model.encode_features(asr_model.extract_features(rs(x, lengths=al)), al, sample_rate=8000)
    for other in (b, c):
        assert torch.equal(a["encoder_out"], other["encoder_out"]) and torch.equal(a["speaker_out"], other["speaker_out"])
        assert torch.equal(a["encoder_padding_mask"], other["encoder_padding_mask"])
    assert bool(a["encoder_padding_mask"][1].any()) and not bool(a["encoder_padding_mask"][0].any())


def test_no_sample_rate_is_todays_call(sd_model, asr_model):
    from tal_asrd_amd import synth
    x = torch.from_numpy(synth.synth_audio_batch(1, 10 * 16000, 9)).to(dev())
    al = torch.tensor([160000])
    with torch.no_grad():
        f0, i0 = sd_model.speaker_ids(x)
        for sr in (None, 16000):
            f, i = sd_model.speaker_ids(x, sample_rate=sr)
            assert torch.equal(f, f0) and torch.equal(i, i0)
            assert "_resamplers" not in sd_model.__dict__ or sr not in sd_model.__dict__["_resamplers"]
        e0 = asr_model.encode(x.half(), al)
        for sr in (None, 16000):
            e = asr_model.encode(x.half(), al, sample_rate=sr)
            assert torch.equal(e["encoder_out"], e0["encoder_out"]) and torch.equal(e["encoder_padding_mask"], e0["encoder_padding_mask"])
        s0 = sd_model.encode(x, al)
        s1 = sd_model.encode(x, al, sample_rate=16000)
        assert torch.equal(s0["encoder_out"], s1["encoder_out"])


def test_errors(sd_model):
    from tal_asrd_amd import NativeError, Resample
    pcm = _pcm(2, 16000, 4)
    with pytest.raises(NativeError, match="Resample"):
        sd_model.speaker_ids(pcm.to(dev()))                               # int16 without a sample rate
    with pytest.raises(NativeError, match="Resample"):
        sd_model.speaker_ids(pcm.to(dev()), sample_rate=16000)
    with pytest.raises(NativeError):
        list(sd_model.speaker_ids_stream([pcm]))
    with pytest.raises(NativeError):
        Resample(44100, 16000)(pcm)                                       # a CPU tensor
    with pytest.raises(NativeError):
        Resample(44100, 16000)(pcm.to(dev()).to(torch.int32))
    with pytest.raises(NativeError, match="2\\^20"):
        Resample(1048573, 1048575)                                        # 2^20 - 1 phases x 13 taps: beyond the plan cap
    with pytest.raises(NativeError, match="2\\^20"):
        sd_model.speaker_ids(pcm.to(dev()), sample_rate=1048573)
