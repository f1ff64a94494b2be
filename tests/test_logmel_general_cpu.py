"""CPU checks of the general log-mel front-end (LogMelSpec(sr, n_mels), SDModel / ASRModel(n_mels=...)): constructors and
state_dict keys against the reference's (mel_variants_keys.json), the C ABI's frame count and plan sizes, the limits, and the
test's own yardstick (tests/_logmel_general_ref.py) against the oracle at the default shape."""
import json
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN
from tests import _logmel_general_ref as G


def _keys():
    return json.load(open(os.path.join(GOLDEN, "mel_variants_keys.json")))


def _ctors(models):
    c = {
        "SDModel_n40": lambda: models.SDModel(n_mels=40),
        "SDModel_n64": lambda: models.SDModel(n_mels=64),
        "ASRModel_2x_spk_n40": lambda: models.ASRModel("2x", n_mels=40, num_speakers=6008, use_speaker_head=True),
    }
    for sr in (8000, 22050, 48000):
        for nm in (40, 128):
            c["LogMelSpec_sr%d_n%d" % (sr, nm)] = (lambda sr=sr, nm=nm: models.LogMelSpec(sr=sr, n_mels=nm))
    return c


def test_mel_variants_construct_with_reference_keys():
    from tal_asrd_amd import models, synth
    ref = _keys()
    ctors = _ctors(models)
    assert sorted(ctors) == sorted(ref)
    for name, ctor in ctors.items():
        m = ctor()
        own = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert own == ref[name], name
        sd = synth.fill_state_dict({k: tuple(s) for k, s in ref[name]})
        full = m.state_dict()                      # (fill_state_dict leaves the front-end's buffers as they are built)
        full.update({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
        m.load_state_dict(full, strict=True)


def test_frames_and_general_plan_bytes():
    from tal_asrd_amd import _native as N
    lib = N.lib()
    for L, hop in ((480000, 160), (15999, 160), (0, 1), (1, 1), (123457, 80), (2048, 2048), (2047, 2048), (1 << 40, 441)):
        assert lib.tal_logmel_frames(L, hop) == 1 + L // hop
    assert lib.tal_logmel_frames(480000, 160) == lib.tal_logmel_num_frames(480000)
    for n_fft, n_mels in ((32, 1), (400, 80), (551, 40), (1200, 16), (2048, 256), (200, 128)):
        assert lib.tal_logmel_general_plan_bytes(n_fft, n_mels) > 0
    for n_fft, n_mels in ((31, 80), (2049, 80), (400, 0), (400, 257)):
        assert lib.tal_logmel_general_plan_bytes(n_fft, n_mels) == 0
    assert lib.tal_logmel_general_workspace_bytes(400, 160, 2, 48000) >= (2 * 19 + 2) * 8


def test_limits_raise_with_the_limit_named():
    from tal_asrd_amd import NativeError, models
    with pytest.raises(NativeError, match="n_fft=5000 outside 32..2048"):
        models.LogMelSpec(sr=200000)
    with pytest.raises(NativeError, match="n_mels=300 outside 1..256"):
        models.LogMelSpec(n_mels=300)
    with pytest.raises(NativeError, match=r"C % 4 == 0"):
        models.SDModel(n_mels=23)
    with pytest.raises(NativeError, match=r"C % 4 == 0"):
        models.ASRModel("1x", n_mels=23)
    models.LogMelSpec(sr=16000, n_mels=23)          # the front-end alone takes odd mel counts
    models.LogMelSpec(sr=1280, n_mels=1)           # n_fft = 32, hop = 12


def test_plan_init_rejects_out_of_range_shapes_before_touching_memory():
    from tal_asrd_amd import _native as N
    lib = N.lib()
    assert lib.tal_logmel_general_plan_init(None, 400, 160, None, 80, None, None) == -1
    assert b"null pointer" in lib.tal_last_error()
    assert lib.tal_logmel_general_fwd(None, 400, 160, 80, None, 0, 1, 1000, 1e-6, 1, None, None, None, None, 0, None) == -1
    assert b"null pointer" in lib.tal_last_error()
    # out-of-range shapes: rejected by argument checks that run before any pointer is used (these pointers are never valid)
    p = 4096
    for n_fft, hop, n_mels, limit in ((31, 10, 80, b"n_fft=31"), (2049, 160, 80, b"n_fft=2049"), (400, 0, 80, b"hop=0"),
                                      (400, 401, 80, b"hop=401"), (400, 160, 0, b"n_mels=0"), (400, 160, 257, b"n_mels=257")):
        assert lib.tal_logmel_general_plan_init(p, n_fft, hop, p, n_mels, p, None) == -1
        assert limit in lib.tal_last_error(), lib.tal_last_error()
        assert lib.tal_logmel_general_fwd(p, n_fft, hop, n_mels, p, 0, 1, 100000, 1e-6, 1, p, p, p, p, 1 << 20, None) == -1
        assert limit in lib.tal_last_error(), lib.tal_last_error()
    # L must exceed n_fft / 2 (reflect padding)
    assert lib.tal_logmel_general_fwd(p, 1200, 480, 128, p, 0, 1, 600, 1e-6, 1, p, p, p, p, 1 << 20, None) == -1
    assert b"L>600" in lib.tal_last_error(), lib.tal_last_error()


def test_option_is_listed_and_off_by_default():
    from tal_asrd_amd import _native as N
    assert N.get_option("logmel_general") == 0


def test_restatements_match_the_oracle_at_the_default_shape():
    from oracle import tal_oracle as O
    from tal_asrd_amd import synth
    audio = synth.synth_audio_batch(2, 16000, 11)
    win, fb = G.buffers(16000, 80)
    assert G.shape_for(16000) == (400, 160)
    np.testing.assert_array_equal(win.numpy(), O.hann_window().numpy())
    np.testing.assert_array_equal(fb.numpy(), O.mel_filterbank().numpy())
    got32 = G.logmel_f32(audio, win, fb, 160).numpy()
    np.testing.assert_allclose(got32, O.logmel(audio).numpy(), atol=1e-5, rtol=0)
    got64 = G.logmel_f64(audio, G.hann_f64(400), fb.double().numpy(), 160)
    np.testing.assert_allclose(got64, O.logmel_f64(audio), atol=1e-9, rtol=0)
    part = G.logmel_f64_frames(audio[1], G.hann_f64(400), fb.double().numpy(), 160, 30, 50)
    np.testing.assert_allclose(part, O.logmel_f64_frames(audio[1], 30, 50), atol=1e-9, rtol=0)
