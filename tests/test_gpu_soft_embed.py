"""Softmax-weighted embeddings without the logits (csrc/soft_embed.hip: tal_soft_embed_fwd, tal_soft_embed_rows, tal_lm_soft_embed_fwd)
against the float64 model of tests/_soft_embed_ref.py: both forms (generic = dense layer + row kernel + dense layer, fused = the
two-product MFMA kernel with online softmax), the fused form at launch sizes that put the boundaries between workgroups inside a row
block, values aliased to the keys and a separate asymmetric matrix, guard rows behind every output and guard bytes behind the
workspace, exact cases bit-equal, the four orders of the running maximum, masked columns, repeatability, dispatch and refusals, the
LM head entry point, and SDModel.speaker_soft_embeds / System.speaker_token_embeds against the reference's own models
(tests/golden/sd_30s_soft.npz, asr_soft_embed.npz)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import _soft_embed_ref as R
from tests.conftest import GOLDEN, golden, has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

LOGIT_TOL = 1e-3      # BASELINE.json north_star: logits within 1e-3 fp32 (as tests/test_gpu_head_topk.py)
GRIDS = (0, 1, 2, 3, 7)
GUARD = 4             # rows behind every output
F_GUARD = 12345.0


def dev():
    return torch.device("cuda:0")


class _Options:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from tal_asrd_amd import _native as N
        for k, v in self.kw.items():
            N.set_option(k, v)

    def __exit__(self, *a):
        from tal_asrd_amd import _native as N
        for k in self.kw:
            N.set_option(k, 0)


def _guarded(M, D):
    return (torch.full((M + GUARD, D), F_GUARD, dtype=torch.float32, device=dev()),
            torch.full((M + GUARD,), F_GUARD, dtype=torch.float32, device=dev()))


def _unguard(M, out, lse):
    torch.cuda.synchronize()
    assert bool((out[M:] == F_GUARD).all()) and bool((lse[M:] == F_GUARD).all()), "guard rows written"
    return out[:M].cpu().numpy(), lse[:M].cpu().numpy()


def soft_embed(feat, W, b, values, form, grid=0, want_lse=True, ws_bytes=None):
    """tal_soft_embed_fwd through the C ABI (feat [M, ldf], the row pitch is its width; values None: values = W) with guard rows
    behind out / lse and guard bytes behind the workspace."""
    from tal_asrd_amd import _native as N
    lib = N.lib()
    M, ldf = feat.shape
    S, E = W.shape
    D = E if values is None else values.shape[1]
    out, lse = _guarded(M, D)
    with _Options(soft_embed_form=form, soft_embed_grid=grid):
        nws = lib.tal_soft_embed_workspace_bytes(M, S, E, D) if ws_bytes is None else ws_bytes
        ws = torch.full((nws + 256,), 0xAB, dtype=torch.uint8, device=dev())
        N.check(lib.tal_soft_embed_fwd(N.ptr(feat), M, ldf, E, N.ptr(W), N.ptr(b), S, N.ptr(values), D, N.ptr(out),
                                       N.ptr(lse) if want_lse else None, N.ptr(ws), nws, N.stream_handle()), "tal_soft_embed_fwd")
    res = _unguard(M, out, lse)
    assert bool((ws[nws:] == 0xAB).all()), "bytes behind the workspace written"
    return res


def _to_dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev()) for a in arrays]


def _fused_ok(W, values):
    return W.shape[1] in R.FUSED_WIDTHS and (values is None or values.shape[1] == W.shape[1])


def _runs(feat, W, b, values):
    yield "generic", soft_embed(feat, W, b, values, 1)
    if _fused_ok(W, values):
        for g in GRIDS:
            yield "fused grid %d" % g, soft_embed(feat, W, b, values, 2, g)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_both_forms_against_the_model(name):
    feat_h, W_h, b_h, V_h, ref_alias, ref_sep = R.build(name)
    feat, W, b, V = _to_dev(feat_h, W_h, b_h, V_h)
    worst = 0.0
    for ref, values in ((ref_alias, None), (ref_sep, V)):
        if ref is None:
            continue
        for what, (out, lse) in _runs(feat, W, b, values):
            ratio = R.error_ratio(ref, out)
            worst = max(worst, ratio)
            print("%s %s %s: error / bound = %.3f" % (name, "separate" if ref.separate else "aliased", what, ratio))
            assert R.compare(ref, out, lse) == [], (name, ref.separate, what)
    print("soft_embed worst error-to-bound ratio of %s: %.4f" % (name, worst))


def test_null_bias_is_zeros_and_null_lse():
    feat_h, W_h, b_h, V_h, _, _ = R.build("random-129-300-64")
    feat, W, b, V = _to_dev(feat_h, W_h, b_h, V_h)
    zeros = torch.zeros_like(b)
    ref = R.make_ref(feat_h, W_h, None, V_h)
    for form, grid in ((1, 0), (2, 0), (2, 3)):
        none = soft_embed(feat, W, None, V, form, grid)
        assert R.compare(ref, *none) == [], (form, grid)
        zero = soft_embed(feat, W, zeros, V, form, grid)
        assert np.array_equal(_bits(none[0]), _bits(zero[0])) and np.array_equal(_bits(none[1]), _bits(zero[1])), (form, grid)
        full = soft_embed(feat, W, b, V, form, grid)
        out, lse = soft_embed(feat, W, b, V, form, grid, want_lse=False)        # (_unguard: a NULL output stays untouched as a whole)
        assert np.array_equal(_bits(out), _bits(full[0])) and (lse == F_GUARD).all(), (form, grid)


def test_three_calls_are_bit_identical():
    for name in R.REPEAT_CASES:
        feat_h, W_h, b_h, V_h, ref_alias, ref_sep = R.build(name)
        feat, W, b, V = _to_dev(feat_h, W_h, b_h, V_h)
        for form, grid in ((1, 0), (2, 0), (2, 7)):
            for ref, values in ((ref_alias, None), (ref_sep, V)):
                first = soft_embed(feat, W, b, values, form, grid)
                assert R.compare(ref, *first) == [], (name, form, grid)
                for _ in range(2):
                    again = soft_embed(feat, W, b, values, form, grid)
                    for a, c in zip(first, again):
                        assert np.array_equal(_bits(a), _bits(c)), (name, form, grid)


def test_generic_form_in_small_pieces():
    """The generic form takes as many rows at a time as its workspace holds: values^T and three rows' worth gives the bits of the
    full workspace (the rows do not interact), with the bytes behind it untouched."""
    feat_h, W_h, b_h, V_h, _, ref = R.build("random-33-301-128-n301")
    feat, W, b, V = _to_dev(feat_h, W_h, b_h, V_h)
    full = soft_embed(feat, W, b, V, 1)
    small = soft_embed(feat, W, b, V, 1, ws_bytes=(128 + 3) * 304 * 4)
    assert R.compare(ref, *small) == []
    assert np.array_equal(_bits(full[0]), _bits(small[0])) and np.array_equal(_bits(full[1]), _bits(small[1]))


def test_no_rows_and_the_refusals():
    from tal_asrd_amd import NativeError, _native as N, ops
    lib = N.lib()
    feat_h, W_h, b_h, V_h, _, ref = R.build("random-129-300-64")
    feat, W, b, V = _to_dev(feat_h, W_h, b_h, V_h)
    out, lse = _guarded(ref.M, 64)
    ws = torch.empty(max(lib.tal_soft_embed_workspace_bytes(ref.M, 300, 64, 64), 1 << 20), dtype=torch.uint8, device=dev())
    args = (N.ptr(W), N.ptr(b), 300, N.ptr(V), 64, N.ptr(out), N.ptr(lse), N.ptr(ws))
    # M == 0
    assert lib.tal_soft_embed_fwd(N.ptr(feat), 0, 64, 64, *args, ws.numel(), N.stream_handle()) == 0
    assert lib.tal_soft_embed_rows(N.ptr(feat), 0, 64, N.ptr(V), 64, N.ptr(out), N.ptr(lse), N.ptr(ws), ws.numel(), N.stream_handle()) == 0
    # a short workspace, either form: refused, nothing launched
    for form in (1, 2):
        with _Options(soft_embed_form=form):
            assert lib.tal_soft_embed_fwd(N.ptr(feat), ref.M, 64, 64, *args, 64, N.stream_handle()) == -2
            assert b"workspace 64 <" in lib.tal_last_error()
            assert lib.tal_soft_embed_fwd(N.ptr(feat), ref.M, 64, 64, *args[:-1], None, ws.numel(), N.stream_handle()) == -2
    x = torch.zeros(8, 300, device=dev())
    assert lib.tal_soft_embed_rows(N.ptr(x), 8, 300, N.ptr(V), 64, N.ptr(out), N.ptr(lse), N.ptr(ws), 64, N.stream_handle()) == -2
    # null pointers, bad shapes
    assert lib.tal_soft_embed_fwd(N.ptr(feat), ref.M, 64, 64, N.ptr(W), N.ptr(b), 300, N.ptr(V), 64, None, None, N.ptr(ws), ws.numel(),
                                  N.stream_handle()) == -1 and b"null pointer" in lib.tal_last_error()
    assert lib.tal_soft_embed_fwd(N.ptr(feat), ref.M, 60, 64, *args, ws.numel(), N.stream_handle()) == -1 and b"bad shape" in lib.tal_last_error()
    # the fused form where the shape does not allow it is an error, not a fallback: widths without a fused form (E = 32; D != E),
    # a pitch off the 16-byte grid, an operand off it
    f32, w32, b32, v20 = _to_dev(*R.build("random-33-300-32")[:4])
    with _Options(soft_embed_form=2):
        assert lib.tal_soft_embed_fwd(N.ptr(f32), 33, 32, 32, N.ptr(w32), N.ptr(b32), 300, N.ptr(v20), 20, N.ptr(out), None, N.ptr(ws), ws.numel(),
                                      N.stream_handle()) == -1 and b"fused form" in lib.tal_last_error()
        assert lib.tal_soft_embed_fwd(N.ptr(f32), 33, 32, 32, N.ptr(w32), N.ptr(b32), 300, None, 32, N.ptr(out), None, N.ptr(ws), ws.numel(),
                                      N.stream_handle()) == -1 and b"fused form" in lib.tal_last_error()
        assert lib.tal_soft_embed_fwd(N.ptr(feat), 8, 64, 64, N.ptr(W), N.ptr(b), 300, N.ptr(v20), 20, N.ptr(out), None, N.ptr(ws), ws.numel(),
                                      N.stream_handle()) == -1 and b"fused form" in lib.tal_last_error()
        wide = torch.zeros(8, 66, device=dev())
        assert lib.tal_soft_embed_fwd(N.ptr(wide), 8, 66, 64, *args, ws.numel(), N.stream_handle()) == -1 and b"fused form" in lib.tal_last_error()
        assert lib.tal_soft_embed_fwd(C.c_void_p(feat.data_ptr() + 4), 8, 64, 64, *args, ws.numel(), N.stream_handle()) == -1
        with pytest.raises(NativeError, match="fused form"):
            ops.soft_embed(f32, w32, b32, v20)
    _unguard(0, out, lse)             # nothing was written by any of these
    # auto dispatch gives one of the two forms' results -- on both sides of its row threshold (128 rows, profiles/soft_embed.txt: the
    # generic form below it, the fused form from it) -- and a width the fused kernel does not take runs the generic form
    for rows in (127, 128, 129):
        fr = feat[:rows].contiguous()
        auto = soft_embed(fr, W, b, V, 0)
        same = [all(np.array_equal(_bits(a), _bits(c)) for a, c in zip(auto, soft_embed(fr, W, b, V, f))) for f in (1, 2)]
        assert any(same), rows
        differ = not all(same)
        assert not differ or same == ([True, False] if rows < 128 else [False, True]), (rows, same)
    got = ops.soft_embed(f32.reshape(1, 33, 32), w32, b32, v20, want_lse=True)
    assert [tuple(o.shape) for o in got] == [(1, 33, 20), (1, 33)]
    assert R.compare(R.build("random-33-300-32")[5], got[0][0].cpu().numpy(), got[1][0].cpu().numpy()) == []
    alias = ops.soft_embed(feat, W, b)
    assert tuple(alias.shape) == (ref.M, 64) and R.compare(R.build("random-129-300-64")[4], alias.cpu().numpy()) == []
    with pytest.raises(NativeError):
        ops.soft_embed(feat.double(), W, b)
    with pytest.raises(NativeError):
        ops.soft_embed(feat, W, b, V[:-1])


@pytest.mark.parametrize("name", sorted(R.ROWS_CASES))
def test_soft_embed_rows_on_materialised_matrices(name):
    from tal_asrd_amd import _native as N, ops
    lib = N.lib()
    x_h, V_h, ref = R.build_rows(name)
    x, V = _to_dev(x_h, V_h)
    keep = x.clone()
    out, lse = _guarded(ref.M, ref.D)
    nws = lib.tal_soft_embed_rows_workspace_bytes(ref.M, ref.N, ref.D)
    ws = torch.full((nws + 256,), 0xAB, dtype=torch.uint8, device=dev())
    N.check(lib.tal_soft_embed_rows(N.ptr(x), ref.M, ref.N, N.ptr(V), ref.D, N.ptr(out), N.ptr(lse), N.ptr(ws), nws, N.stream_handle()),
            "tal_soft_embed_rows")
    got = _unguard(ref.M, out, lse)
    assert bool((ws[nws:] == 0xAB).all()) and torch.equal(x, keep)
    print("%s: error / bound = %.3f" % (name, R.error_ratio(ref, got[0])))
    assert R.compare(ref, *got) == [], name
    o2, l2 = ops.soft_embed_rows(x.reshape(1, ref.M, ref.N), V, want_lse=True)
    assert np.array_equal(_bits(o2[0].cpu().numpy()), _bits(got[0])) and np.array_equal(_bits(l2[0].cpu().numpy()), _bits(got[1]))


# ------------------------------------------------------------------ the models
VARIANTS = {"2x_tok": dict(model_type="2x", num_speakers=6008, vocab_size=10000, use_speaker_head=False),
            "1x_e0": dict(model_type="1x", num_speakers=6008, vocab_size=10000, use_speaker_head=True, embed_size=0),
            "2x_spk": dict(model_type="2x", num_speakers=6008, vocab_size=10000, use_speaker_head=True)}
_models = {}


def _model(tag):
    """The variant with the synthetic weights, built once per session."""
    if tag not in _models:
        from tal_asrd_amd import ASRModel, synth
        keys = json.load(open(os.path.join(GOLDEN, "state_dict_keys.json")))["ASRModel_" + tag]
        m = ASRModel(**VARIANTS[tag])
        own = m.state_dict()
        for k, v in synth.fill_state_dict({k: tuple(s) for k, s in keys}).items():
            assert k in own, k
            own[k] = torch.from_numpy(np.array(v, copy=True))
        m.load_state_dict(own)
        _models[tag] = m.to(dev())
    return _models[tag]


@pytest.fixture(scope="module")
def sd_model(sd_weights):
    from tal_asrd_amd import SDModel
    model = SDModel()
    own = model.state_dict()
    for k, v in sd_weights.items():
        assert k in own, k
        own[k] = torch.from_numpy(np.array(v, copy=True))
    model.load_state_dict(own)
    return model.to(dev())


def _lm_soft_embed(m, rows, col_begin, form, grid=0):
    from tal_asrd_amd import _native as N, decoder
    lib = N.lib()
    M, D = rows.shape
    emb = m.embedding.weight
    V, E0 = emb.shape
    pt = decoder._proj_t(m) if m.embed_size else None
    out, lse = _guarded(M, E0)
    with _Options(soft_embed_form=form, soft_embed_grid=grid):
        nws = lib.tal_lm_soft_embed_workspace_bytes(M, D, E0, V, col_begin)
        ws = torch.full((nws + 256,), 0xAB, dtype=torch.uint8, device=dev())
        N.check(lib.tal_lm_soft_embed_fwd(N.ptr(rows), M, D, D, N.ptr(pt), E0, N.ptr(emb), V, col_begin, N.ptr(out), N.ptr(lse), N.ptr(ws),
                                          nws, N.stream_handle()), "tal_lm_soft_embed_fwd")
    res = _unguard(M, out, lse)
    assert bool((ws[nws:] == 0xAB).all())
    return res


def _lm_ref(m, rows, col_begin):
    """The float64 model of the tied head's columns [col_begin, V) on the hidden rows [M, D], with the two-stage logit bound of
    tests/test_gpu_xent.py: the projected row t carries gamma_{D+2} |h| |P|, which the head multiplies by |emb| on top of its own
    gamma_{E0+2} |t| |emb|."""
    h64 = rows.double().cpu().numpy()
    emb = m.embedding.weight.detach().double().cpu().numpy()[col_begin:]
    if m.embed_size:
        P = m.embedding_proj.weight.detach().double().cpu().numpy()           # [D, E0]: t = h . P
        t = h64 @ P
        dt = R.gamma(P.shape[0] + 2) * (np.abs(h64) @ np.abs(P))
    else:
        t, dt = h64, np.zeros_like(h64)
    B = R.gamma(emb.shape[1] + 2) * (np.abs(t) @ np.abs(emb).T) + (1 + 1e-6) * (dt @ np.abs(emb).T)
    return R.Ref(t @ emb.T, np.zeros(emb.shape[0]), B, emb, emb, False, False)


@pytest.mark.parametrize("tag", ("2x_tok", "1x_e0"))
def test_lm_soft_embed_against_the_model(tag):
    """tal_lm_soft_embed_fwd on random hidden rows: E0 = 64 with the projection (both forms, several grids), no projection and
    D = 256 (the generic form; the fused form is refused there)."""
    from tal_asrd_amd import _native as N
    m = _model(tag)
    D = m.decoder.layers[0].linear1.in_features
    first = m.embedding.weight.shape[0] - 6008       # (2x_tok: the 10000 text tokens; 1x_e0: 6008 of its 10000 columns)
    rows = torch.randn(37, D, generator=torch.Generator().manual_seed(5)).to(dev())
    ref = _lm_ref(m, rows, first)
    runs = [(1, 0)] + ([(2, g) for g in (0, 3)] if m.embed_size else [])
    for form, grid in runs:
        out, lse = _lm_soft_embed(m, rows, first, form, grid)
        print("lm_soft_embed %s form %d grid %d: error / bound = %.3f" % (tag, form, grid, R.error_ratio(ref, out)))
        assert R.compare(ref, out, lse) == [], (tag, form, grid)
    if not m.embed_size:
        with _Options(soft_embed_form=2):
            with pytest.raises(N.NativeError, match="fused form"):
                _lm_soft_embed(m, rows, first, 2)


def test_speaker_soft_embeds_on_the_30_second_fixture(sd_model):
    """SDModel.speaker_soft_embeds against the reference model's own logits (tests/golden/sd_30s_soft.npz, recorded by
    make_golden_soft_embed.py): soft within expm1(2 LOGIT_TOL) max |values| -- logits that differ by at most LOGIT_TOL move every
    probability by a factor within exp(+-2 LOGIT_TOL), and sum_s p_s |values[s, d]| <= max |values| -- lse within 2 LOGIT_TOL; the
    features are speaker_ids' features bit for bit; and the materialised route (want_logits=True, then softmax and matmul in float64 on
    the same device features) is matched to the model's own tolerance, in both forms."""
    from tal_asrd_amd import synth
    g = golden("sd_30s_soft")
    audio = torch.from_numpy(synth.synth_audio_batch(1, int(g["audio_len"]), int(g["audio_seed"]))).to(dev())
    feat0, ids0, logits = sd_model.speaker_ids(audio, want_logits=True)
    table, bias = sd_model.spk_logit_proj.weight.detach(), sd_model.spk_logit_proj.bias.detach()
    bound = np.expm1(2 * LOGIT_TOL) * float(g["max_abs_values"])
    assert abs(float(table.abs().max()) - float(g["max_abs_values"])) < 1e-6
    route = (torch.softmax(logits.double(), dim=-1) @ table.double()).cpu().numpy().reshape(-1, 128)
    ref = R.make_ref(feat0.cpu().numpy().reshape(-1, 128), table.cpu().numpy(), bias.cpu().numpy(), None)
    for form in (1, 2):
        with _Options(soft_embed_form=form):
            feat, soft, lse = sd_model.speaker_soft_embeds(audio)
        assert torch.equal(feat, feat0)
        assert soft.shape == feat0.shape and lse.shape == ids0.shape and soft.dtype == torch.float32
        soft, lse = soft.cpu().numpy().reshape(-1, 128), lse.cpu().numpy().reshape(-1)
        err = np.abs(soft - g["soft"]).max()
        print("speaker_soft_embeds form %d: max |soft - reference| = %.3e (bound %.3e), error / model bound = %.3f, "
              "max |soft - materialised route| = %.3e" % (form, err, bound, R.error_ratio(ref, soft), np.abs(soft - route).max()))
        assert err <= bound, form
        np.testing.assert_allclose(lse, g["lse"], atol=2 * LOGIT_TOL, rtol=0)
        assert R.compare(ref, soft, lse) == [], form
        assert (np.abs(soft - route) <= ref.tol).all(), form
    mel, mean = sd_model.logmelspec.forward_unsubtracted(audio)
    f1, s1, l1 = sd_model.speaker_soft_embeds_from_logmel(mel, mean)
    assert torch.equal(f1, feat0) and R.compare(ref, s1.cpu().numpy().reshape(-1, 128), l1.cpu().numpy().reshape(-1)) == []


class _Tok:
    eos_token_id, bos_token_id, pad_token_id = 1, 0, 2

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_speaker_token_embeds_against_the_reference():
    """System.speaker_token_embeds against the reference's gen_embed.py:83-99 on its own ASRModel (tests/golden/asr_soft_embed.npz):
    positions and speaker ids identical (the speaker token in the padded tail is ignored), embeddings within
    expm1(2 LOGIT_TOL) max |values|, in both forms; a model with a speaker head raises; no speaker token gives empty tensors; the
    no-projection variant (embed_size=0) runs the generic form."""
    from tal_asrd_amd import NativeError, synth
    from tal_asrd_amd.system import System
    g = golden("asr_soft_embed")
    V0 = int(g["vocab_size"])
    m = _model("2x_tok")
    lens = [int(x) for x in g["audio_lens"]]
    audio = torch.from_numpy(synth.synth_audio_batch(2, lens[0], int(g["audio_seed"]), lens=lens)).to(dev())
    y, y_mask = (torch.from_numpy(g[k]).to(dev()) for k in ("y", "y_mask"))
    system = System(m, tokenizer=_Tok(V0))
    bound = np.expm1(2 * LOGIT_TOL) * float(g["max_abs_values"])
    assert int(((g["y"][:, 1:] >= V0) & ~g["y_mask"][:, 1:]).sum()) == 1          # the one in the padded tail
    for form in (1, 2):
        with _Options(soft_embed_form=form):
            pos, ids, emb = system.speaker_token_embeds(audio, torch.tensor(lens), y, y_mask)
        assert pos.dtype == torch.int64 and ids.dtype == torch.int64 and emb.dtype == torch.float32 and emb.is_cuda
        np.testing.assert_array_equal(pos.cpu().numpy(), g["positions"])
        np.testing.assert_array_equal(ids.cpu().numpy(), g["speaker_ids"])
        err = np.abs(emb.cpu().numpy() - g["embeds"]).max()
        print("speaker_token_embeds form %d: max |embeds - reference| = %.3e (bound %.3e)" % (form, err, bound))
        assert emb.shape == g["embeds"].shape and err <= bound, form
    # the model-level entry point on the same encoder output, unmasked: the padded tail's token is one more position
    enc = m.encode(audio, torch.tensor(lens))
    pos_all, ids_all, emb_all = m.speaker_token_embeds(y[:, :-1], y[:, 1:], enc, V0)
    assert pos_all.shape[0] == g["positions"].shape[0] + 1 and emb_all.shape == (pos_all.shape[0], 64)
    # no speaker token at all
    plain = torch.clamp(y, max=V0 - 1)
    pos0, ids0, emb0 = system.speaker_token_embeds(audio, torch.tensor(lens), plain, y_mask)
    assert tuple(pos0.shape) == (0, 2) and tuple(ids0.shape) == (0,) and tuple(emb0.shape) == (0, 64)
    # a speaker-head model has no speaker tokens
    with pytest.raises(NativeError, match="speaker"):
        _model("2x_spk").speaker_token_embeds(y[:, :-1], y[:, 1:], enc, V0)
