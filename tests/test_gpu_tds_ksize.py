"""TDS at kernel sizes other than 21 on the GPU (csrc/gconv_general.hip and its dispatch in tal_tds_fwd).

  bit identity at k = 21    tal_gconv_s2_k_fwd / tal_gconv_res_k_fwd against tal_gconv_s2_fwd / tal_gconv_res_fwd: the encoder's
                            widths at groups 80 and 40, an odd width (runtime-width path), T at the kernel and a 1-hour stage length
  against float64           k in {1, 2*, 3, 5, 7, 11, 15, 20*, 31, 33, 63} (* resize only) x both forms x widths x B in {1, 3} x
                            T in {k, k + 1, ragged, long}; allowed error max(4 * e32, floor), e32 the same restatement's error in
                            CPU float32 (tests/_tds_ksize_ref.py); the block conv's zero padding at both true ends of every item
  fixtures                  tds_ksize.npz through TDS / TDSBlock.forward; sd_k15_30s.npz through an SDModel whose encoder is a
                            kernel-size-15 TDS; ASRModel('2x') with a k = 15 encoder against the float64 restatement
  whole encoder at k = 21   option gconv_general on / off bit-identical under TAL_TDS_EXACT_F32; the default output unchanged
  tiling, determinism       tal_tds_tiled_fwd at k = 15 against the one-call form; a 5-minute speaker_ids call repeated
Fixtures only: nothing here reads the reference tree."""
import ctypes as C

import numpy as np
import pytest
import torch

from tal_asrd_amd import _native as N, ops, synth
from tal_asrd_amd.models import ASRModel, SDModel, TDS, TDSBlock
from tests import _tds_ksize_ref as R
from tests.conftest import golden

pytestmark = pytest.mark.gpu

SIZES, DEPTHS = [80, 800, 1120, 1440], [2, 3, 6]


def dev():
    return torch.device("cuda:0")


def _rand(name, shape, bound=1.0):
    return torch.from_numpy(synth.synth_tensor(name, shape, bound))


def _conv_params(tag, c_in, c_out, groups, k):
    w = _rand(tag + "/w", (c_out, c_in // groups, k), 1.0 / np.sqrt(c_in // groups * k))
    b = _rand(tag + "/b", (c_out,), 0.1)
    return w, b


def _s2_k(x, wp, b, c_out, groups, k):
    return ops.gconv_s2_k(x, wp, b, c_out, groups, k)


def _res_k(x, wp, b, alpha, groups, k):
    return ops.gconv_res_k(x, wp, b, alpha, groups, k)


@pytest.mark.parametrize("groups", [80, 40])
def test_k21_bit_identical_to_the_specialised_kernels(groups):
    lib = N.lib()
    for cig, cog in ((1, 10), (10, 14), (14, 18), (3, 5)):
        w, b = _conv_params("bit/s2/%d/%d" % (cig, cog), cig * groups, cog * groups, groups, 21)
        wp, bd = ops.pack_gconv_weight(w.to(dev()), groups), b.to(dev())
        for B, T in ((1, 21), (3, 22), (2, 23), (1, 2000)):
            x = _rand("bit/x/%d/%d" % (cig, T), (B, T, cig * groups)).to(dev())
            assert torch.equal(_s2_k(x, wp, bd, cog * groups, groups, 21), ops.gconv_s2(x, wp, bd, cog * groups, groups)), (cig, cog, B, T)
    for cg in (10, 14, 18, 7):
        w, b = _conv_params("bit/res/%d" % cg, cg * groups, cg * groups, groups, 21)
        wp, bd = ops.pack_gconv_weight(w.to(dev()), groups), b.to(dev())
        for B, T in ((1, 1), (3, 21), (2, 22), (1, 2000)):
            x = _rand("bit/xr/%d/%d" % (cg, T), (B, T, cg * groups)).to(dev())
            assert torch.equal(_res_k(x, wp, bd, 0.37, groups, 21), ops.gconv_res(x, wp, bd, 0.37, groups)), (cg, B, T)
    assert lib.tal_version() == 501


def test_k21_bit_identical_at_one_hour_stage_lengths():
    # the 1-hour clip's stage lengths (360001 mel frames -> 179991 -> 89986 -> 44983) at the encoder's widths, groups 80
    g = 80
    for cig, cog, T, stride in ((1, 10, 360001, 2), (10, 14, 179991, 2), (14, 18, 89986, 2),
                                (10, 10, 179991, 1), (14, 14, 89986, 1), (18, 18, 44983, 1)):
        w, b = _conv_params("hour/%d/%d/%d" % (cig, cog, stride), cig * g, cog * g, g, 21)
        wp, bd = ops.pack_gconv_weight(w.to(dev()), g), b.to(dev())
        x = (torch.rand(1, T, cig * g, device=dev(), generator=torch.Generator(device=dev()).manual_seed(T)) * 2 - 1)
        if stride == 2:
            same = torch.equal(_s2_k(x, wp, bd, cog * g, g, 21), ops.gconv_s2(x, wp, bd, cog * g, g))
        else:
            same = torch.equal(_res_k(x, wp, bd, 0.61, g, 21), ops.gconv_res(x, wp, bd, 0.61, g))
        assert same, (cig, cog, T)
        del x
        torch.cuda.empty_cache()


def _check64(got, x, w, b, groups, alpha=None):
    """max |got - ref64| <= max(4 * e32, floor).  e32: the restatement's own error in CPU float32 (torch sums in blocks); floor: the
    a-priori bound of the kernels' recursive fmaf chain, n u max(|b| + sum |w x|) for n = C_in / G * k products (plus one rounding of
    the epilogue) -- for long chains the blocked CPU sum is the more accurate of the two."""
    n = w.shape[1] * w.shape[2]
    if alpha is None:
        r64 = R.gconv_s2_tm(x, w, b, groups, torch.float64)
        r32 = R.gconv_s2_tm(x, w, b, groups, torch.float32)
        mag = R.gconv_s2_tm(x.abs(), w.abs(), b.abs(), groups, torch.float64)
    else:
        r64 = R.gconv_res_tm(x, w, b, alpha, groups, torch.float64)
        r32 = R.gconv_res_tm(x, w, b, alpha, groups, torch.float32)
        mag = abs(alpha) * (R.gconv_res_tm(x.abs(), w.abs(), b.abs(), 1.0, groups, torch.float64) - x.abs().double())
    e32 = float((r32.double() - r64).abs().max())
    u = 2.0 ** -24
    floor = n * u * float(mag.max()) + 2 * u * float(r64.abs().max())
    err = float((got.cpu().double() - r64).abs().max())
    assert got.shape == r64.shape
    assert err <= max(4 * e32, floor), (err, e32, floor)


KS = [1, 2, 3, 5, 7, 11, 15, 20, 31, 33, 63]


@pytest.mark.parametrize("k", KS)
def test_resize_conv_against_float64(k):
    # (groups, C_in / G, C_out / G): the 1 -> 10 channel-major kernel (groups % 20 == 0), the two compile-time widths, a runtime width
    for groups, cig, cog in ((20, 1, 10), (4, 10, 14), (4, 14, 18), (4, 3, 5)):
        w, b = _conv_params("f64/s2/%d/%d/%d" % (k, cig, cog), cig * groups, cog * groups, groups, k)
        wp, bd = ops.pack_gconv_weight(w.to(dev()), groups), b.to(dev())
        for B in (1, 3):
            for T in (k, k + 1, k + 136, 2 * 128 * 3 + k + 5):       # at the kernel, one more, ragged, several tiles
                x = _rand("f64/s2/x/%d/%d/%d/%d" % (k, cig, B, T), (B, T, cig * groups))
                y = _s2_k(x.to(dev()), wp, bd, cog * groups, groups, k)
                assert y.shape[1] == (T - k) // 2 + 1
                _check64(y, x, w, b, groups)


@pytest.mark.parametrize("k", [k for k in KS if k % 2 == 1])
def test_block_conv_against_float64(k):
    for groups, cg in ((4, 10), (4, 14), (4, 18), (4, 7)):
        w, b = _conv_params("f64/res/%d/%d" % (k, cg), cg * groups, cg * groups, groups, k)
        wp, bd = ops.pack_gconv_weight(w.to(dev()), groups), b.to(dev())
        for B in (1, 3):
            for T in (k, k + 1, k + 97, 2 * 256 + k + 3):
                # large values at both true ends of each item: an error in the zero padding shows at once
                x = _rand("f64/res/x/%d/%d/%d/%d" % (k, cg, B, T), (B, T, cg * groups))
                x[:, :2] *= 8
                x[:, -2:] *= 8
                y = _res_k(x.to(dev()), wp, bd, 0.83, groups, k)
                _check64(y, x, w, b, groups, alpha=0.83)


def test_argument_checks():
    x = torch.zeros(1, 30, 40, device=dev())
    w, b = _conv_params("args", 40, 40, 4, 4)
    wp, bd = ops.pack_gconv_weight(w.to(dev()), 4), b.to(dev())
    with pytest.raises(N.NativeError, match="must be odd"):
        _res_k(x, wp, bd, 0.5, 4, 4)
    with pytest.raises(N.NativeError, match="outside 1..63"):
        _s2_k(torch.zeros(1, 100, 40, device=dev()), wp, bd, 40, 4, 64)
    with pytest.raises(N.NativeError, match="too few"):
        _s2_k(x[:, :3], wp, bd, 40, 4, 4)


def _small_tds(k, depths, prefix):
    m = TDS(input_size=8, sizes=[8, 16, 24, 32], depths=depths, kernel_size=k)
    return R.load_synth(m, prefix).to(dev())


@pytest.mark.parametrize("k,depths", [(3, [1, 1, 2]), (11, [1, 1, 2]), (31, [1, 1, 2]), (8, [0, 0, 0])])
def test_tds_ksize_golden(k, depths):
    g = golden("tds_ksize")
    m = _small_tds(k, depths, "tds_k%d." % k)
    y = m(torch.from_numpy(g["tds_k%d_x" % k]).to(dev()))
    np.testing.assert_allclose(y.cpu().numpy(), g["tds_k%d_y" % k], atol=2e-5, rtol=0)


@pytest.mark.parametrize("k", [5, 15])
def test_tdsblock_ksize_golden(k):
    g = golden("tds_ksize")
    m = R.load_synth(TDSBlock(32, k, 8), "block_k%d." % k).to(dev())
    y = m(torch.from_numpy(g["block_k%d_x" % k]).to(dev()))
    np.testing.assert_allclose(y.cpu().numpy(), g["block_k%d_y" % k], atol=2e-5, rtol=0)


def test_grouped_conv_direct_call_uses_its_kernel_size():
    m = _small_tds(11, [1, 1, 2], "tds_k11.")
    x = _rand("direct/x", (2, 50, 8))
    y = m.blocks[0][0](x.to(dev()))
    assert y.shape == (2, (50 - 11) // 2 + 1, 16)
    sd = m.state_dict()
    _check64(y, x, sd["blocks.0.0.weight"].cpu(), sd["blocks.0.0.bias"].cpu(), 8)


def _swap_encoder(model, k):
    """A model whose encoder was replaced by TDS(80, [80, 800, 1120, 1440], [2, 3, 6], kernel_size=k), with synthetic weights."""
    model.encoder = TDS(80, SIZES, DEPTHS, kernel_size=k)
    return R.load_synth(model).to(dev())


@pytest.fixture(scope="module")
def sd_k15():
    return _swap_encoder(SDModel(), 15)


LOGIT_TOL = 1e-3


def test_sd_k15_30s_golden(sd_k15):
    g = golden("sd_k15_30s")
    assert int(g["kernel_size"]) == 15
    audio = torch.from_numpy(synth.synth_audio_batch(1, int(g["audio_len"]), int(g["audio_seed"]))).to(dev())
    with torch.no_grad():
        mel = sd_k15.extract_features(audio)
        enc = sd_k15.encode_features(mel)
        eo = enc["encoder_out"]
        np.testing.assert_allclose(eo[:, g["enc_rows"]].cpu().numpy(), g["enc_sample"], atol=LOGIT_TOL, rtol=0)
        logits = sd_k15.decode(enc)
        np.testing.assert_allclose(logits[:, g["logit_rows"]].cpu().numpy(), g["logit_sample"], atol=LOGIT_TOL, rtol=0)
        np.testing.assert_allclose(logits.max(-1).values.cpu().numpy(), g["logit_max"], atol=LOGIT_TOL, rtol=0)
        np.testing.assert_array_equal(logits.argmax(-1).cpu().numpy(), g["ids"])
        # the product entry point (premean fold and split head are off for k != 21: the plain paths run)
        _, ids, lg = sd_k15.speaker_ids(audio, want_logits=True)
        np.testing.assert_array_equal(ids.cpu().numpy().reshape(g["ids"].shape), g["ids"])
        np.testing.assert_allclose(lg.max(-1).values.cpu().numpy().reshape(g["logit_max"].shape), g["logit_max"], atol=LOGIT_TOL, rtol=0)


def test_sd_k15_batched_ragged_and_stream(sd_k15):
    lens = [160000, 120000]
    audio = torch.from_numpy(synth.synth_audio_batch(2, 160000, 99, lens=lens)).to(dev())
    with torch.no_grad():
        logits, eo = sd_k15(audio, torch.tensor(lens))
        enc = sd_k15.encode(audio, torch.tensor(lens))
        t_out = enc["encoder_out"].shape[1]
        assert logits.shape[:2] == (2, t_out) and torch.equal(eo["encoder_out"], enc["encoder_out"])
        scaled = torch.tensor(lens) // (max(lens) // t_out)
        mask = torch.arange(t_out)[None, :] >= scaled[:, None]
        assert torch.equal(enc["encoder_padding_mask"].cpu(), mask)
        feats = sd_k15.extract_features(audio)
        assert sd_k15.encode_features(feats)["encoder_out"].shape == enc["encoder_out"].shape
        clips = [audio[0:1].cpu(), audio[1:2, :lens[1]].cpu()]
        got = list(sd_k15.speaker_ids_stream(clips))
        assert len(got) == 2
        for clip, (feat, ids) in zip(clips, got):
            _, ids1 = sd_k15.speaker_ids(clip.to(dev()))
            assert torch.equal(ids.reshape(-1), ids1.reshape(-1))


def test_asr_k15_encode_against_float64():
    model = _swap_encoder(ASRModel("2x", num_speakers=6008, vocab_size=10000, use_speaker_head=True), 15)
    lens = [480000, 400000]
    audio = torch.from_numpy(synth.synth_audio_batch(2, 480000, 1234, lens=lens)).to(dev())
    with torch.no_grad():
        mel = model.extract_features(audio)
        enc = model.encode_features(mel, torch.tensor(lens))
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    enc_sd = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
    h64 = R.tds(mel.cpu().transpose(1, 2), enc_sd, 80, DEPTHS, 15, torch.float64).transpose(1, 2)
    ref = h64 @ sd["decoder_proj.weight"].double().T + sd["decoder_proj.bias"].double()
    eo = enc["encoder_out"].cpu().double()
    assert eo.shape == ref.shape
    err = float((eo - ref).abs().max())
    assert err <= 1e-3 * max(1.0, float(ref.abs().max())), err
    t_out = eo.shape[1]
    scaled = torch.tensor(lens) // (max(lens) // t_out)
    assert torch.equal(enc["encoder_padding_mask"].cpu(), torch.arange(t_out)[None, :] >= scaled[:, None])


def _set_option(name, value):
    assert N.lib().tal_set_option(name.encode(), int(value)) == 0


@pytest.fixture(scope="module")
def sd_k21():
    return R.load_synth(SDModel()).to(dev())


@pytest.mark.parametrize("seconds", [30, 300])
def test_gconv_general_option_is_bit_identical_at_k21(sd_k21, seconds):
    audio = torch.from_numpy(synth.synth_audio_batch(1, 16000 * seconds, 1234)).to(dev())
    with torch.no_grad():
        mel = sd_k21.extract_features(audio)
    desc = sd_k21.encoder._descriptor()
    exact = N.TdsDesc.from_buffer_copy(desc)
    exact.flags |= N.TAL_TDS_EXACT_F32
    default_before = ops.tds_forward(desc, mel, SIZES[-1])
    off = ops.tds_forward(exact, mel, SIZES[-1])
    _set_option("gconv_general", 1)
    try:
        on = ops.tds_forward(exact, mel, SIZES[-1])
        general_default = ops.tds_forward(desc, mel, SIZES[-1])
        assert ops.tds_premean_ok(desc, mel) is False
    finally:
        _set_option("gconv_general", 0)
    assert torch.equal(on, off)
    # (the option's non-exact run keeps the dense layers' fp16x3 form: close to the default, not equal)
    assert float((general_default - default_before).abs().max()) < 1e-3
    assert torch.equal(ops.tds_forward(desc, mel, SIZES[-1]), default_before)


def test_tiled_k15_matches_the_one_call_form(sd_k15):
    x = _rand("tiled/x", (1, 6001, 80), 2.0).to(dev())
    desc = sd_k15.encoder._descriptor()
    whole = ops.tds_forward(desc, x, SIZES[-1])
    for tile in (37, 200, 1000):
        tiled = ops.tds_forward_tiled(desc, x, SIZES[-1], tile)
        assert tiled.shape == whole.shape
        assert float((tiled - whole).abs().max()) <= 1e-5, tile


def test_sd_k15_five_minutes_is_deterministic(sd_k15):
    audio = torch.from_numpy(synth.synth_audio_batch(1, 16000 * 300, 7)).to(dev())
    with torch.no_grad():
        a_feat, a_ids, a_lg = sd_k15.speaker_ids(audio, want_logits=True)
        b_feat, b_ids, b_lg = sd_k15.speaker_ids(audio, want_logits=True)
    assert torch.equal(a_ids, b_ids) and torch.equal(a_lg, b_lg) and torch.equal(a_feat, b_feat)
