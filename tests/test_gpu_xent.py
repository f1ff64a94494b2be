"""Teacher-forced scoring without the logits (csrc/xent.hip: tal_xent_rows_fwd, tal_xent_lse_rows, tal_lm_xent_fwd) against the float64
model of tests/_xent_ref.py: both forms (generic = dense layer + row kernel, fused = A-stationary MFMA kernel with online
log-sum-exp, running arg-max and target gather), the fused form at launch sizes that put the boundaries between workgroups inside a
row block, guard rows behind every output and guard bytes behind the workspace, repeatability, the LM head entry point on two model
variants, ASRModel.score against decode / decode_spk, and System.score / validation_step against the reference's own training_step
(tests/golden/asr_score.npz)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import _xent_ref as R
from tests.conftest import GOLDEN, golden, has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

LOGIT_TOL = 1e-3      # BASELINE.json north_star: logits within 1e-3 fp32
GRIDS = (0, 1, 2, 3, 7)
GUARD = 4             # rows behind every output
ID_GUARD, F_GUARD = -7, 12345.0


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


def _guarded(M):
    nll = torch.full((M + GUARD,), F_GUARD, dtype=torch.float32, device=dev())
    lse = torch.full((M + GUARD,), F_GUARD, dtype=torch.float32, device=dev())
    top1 = torch.full((M + GUARD,), ID_GUARD, dtype=torch.int32, device=dev())
    return nll, lse, top1


def _unguard(M, nll, lse, top1):
    torch.cuda.synchronize()
    assert bool((nll[M:] == F_GUARD).all()) and bool((lse[M:] == F_GUARD).all()) and bool((top1[M:] == ID_GUARD).all()), "guard rows written"
    return nll[:M].cpu().numpy(), lse[:M].cpu().numpy(), top1[:M].cpu().numpy()


def xent_rows(feat, W, b, target, form, grid=0, want=(True, True)):
    """tal_xent_rows_fwd through the C ABI (feat [M, ldf], the row pitch is its width) with guard rows behind nll / lse / top1 and
    guard bytes behind the workspace."""
    from tal_asrd_amd import _native as N
    lib = N.lib()
    M, ldf = feat.shape
    S, E = W.shape
    nll, lse, top1 = _guarded(M)
    with _Options(xent_form=form, xent_grid=grid):
        nws = lib.tal_xent_rows_workspace_bytes(M, S, E)
        ws = torch.full((nws + 256,), 0xAB, dtype=torch.uint8, device=dev())
        N.check(lib.tal_xent_rows_fwd(N.ptr(feat), M, ldf, E, N.ptr(W), N.ptr(b), S, N.ptr(target), N.ptr(nll), N.ptr(lse) if want[0] else None,
                                      N.ptr(top1) if want[1] else None, N.ptr(ws), nws, N.stream_handle()), "tal_xent_rows_fwd")
    out = _unguard(M, nll, lse, top1)
    assert bool((ws[nws:] == 0xAB).all()), "bytes behind the workspace written"
    return out


def _to_dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev()) for a in arrays]


def _runs(feat, W, b, target):
    yield "generic", xent_rows(feat, W, b, target, 1)
    if W.shape[1] in R.FUSED_E:
        for g in GRIDS:
            yield "fused grid %d" % g, xent_rows(feat, W, b, target, 2, g)


def _bits(a):
    return a.view(np.int32)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_both_forms_against_the_model(name):
    from tal_asrd_amd import _native as N, ops
    feat_h, W_h, b_h, target_h, ref = R.build(name)
    feat, W, b, target = _to_dev(feat_h, W_h, b_h, target_h)
    E = W_h.shape[1]
    results = {}
    for what, (nll, lse, top1) in _runs(feat, W, b, target):
        assert R.compare(ref, nll, lse, top1) == [], (name, what)
        # lse - nll gives the target's logit back, the value the sum saw: nll >= 0 up to the rounding of the sum and of lse
        fin = np.isfinite(ref.nll) & (ref.target >= 0)
        assert (nll[fin] >= -(ref.N + 64) * R.U - 2 * R.U * np.abs(lse[fin])).all(), (name, what)
        results[what] = (nll, lse, top1)
    # the forms agree with each other within twice the bound (each is within the bound of the same model)
    g_nll, g_lse, g_top1 = results["generic"]
    slack = (ref.N + 64) * R.U
    must = np.ones(ref.M, bool) if ref.exact_valued else ref.clear
    for what, (nll, lse, top1) in results.items():
        assert (np.abs(lse.astype(np.float64) - g_lse) <= 2 * (ref.Bmax + slack)).all(), (name, what)
        fin = np.isfinite(g_nll)
        assert np.array_equal(np.isfinite(nll), fin), (name, what)
        assert (np.abs(nll[fin].astype(np.float64) - g_nll[fin]) <= 2 * (ref.Bt + ref.Bmax + slack)[fin]).all(), (name, what)
        np.testing.assert_array_equal(top1[must], g_top1[must], err_msg="%s: %s vs generic" % (name, what))
    # the row kernel alone on the materialised logits of the dense layer: within the bound of the model of THAT matrix, and of the head's
    logits = ops.linear(feat[:, :E].contiguous(), W, b)
    nll, lse, top1 = _guarded(ref.M)
    N.check(N.lib().tal_xent_lse_rows(N.ptr(logits), ref.M, ref.N, N.ptr(target), N.ptr(nll), N.ptr(lse), N.ptr(top1), N.stream_handle()),
            "tal_xent_lse_rows")
    out = _unguard(ref.M, nll, lse, top1)
    assert R.compare(R.rows_ref(logits.cpu().numpy(), target_h), *out) == [], name
    assert R.compare(ref, *out) == [], name
    assert torch.equal(top1[:ref.M], ops.argmax_rows(logits)), name          # (tal_argmax_rows' rule, ties included)


def test_null_lse_top1_bias():
    feat_h, W_h, b_h, target_h, _ = R.build("random-257-300-64")
    feat, W, b, target = _to_dev(feat_h, W_h, b_h, target_h)
    ref = R.linear_ref(feat_h, W_h, None, target_h)
    assert ref.unclear_share <= R.UNCLEAR_CAP
    for what, out in _runs(feat, W, None, target):
        assert R.compare(ref, *out) == [], what
    for form in (1, 2):
        full = xent_rows(feat, W, b, target, form)
        for want in ((False, True), (True, False), (False, False)):
            nll, lse, top1 = xent_rows(feat, W, b, target, form, want=want)        # (_unguard: a NULL output stays untouched as a whole)
            assert np.array_equal(_bits(nll), _bits(full[0])), (form, want)
            assert np.array_equal(_bits(lse), _bits(full[1])) if want[0] else (lse == F_GUARD).all(), (form, want)
            assert np.array_equal(top1, full[2]) if want[1] else (top1 == ID_GUARD).all(), (form, want)


def test_no_rows_and_the_refusals():
    from tal_asrd_amd import NativeError, _native as N, ops
    lib = N.lib()
    feat_h, W_h, b_h, target_h, ref = R.build("random-257-300-64")
    feat, W, b, target = _to_dev(feat_h, W_h, b_h, target_h)
    nll, lse, top1 = _guarded(ref.M)
    ws = torch.empty(lib.tal_xent_rows_workspace_bytes(ref.M, 300, 64), dtype=torch.uint8, device=dev())
    args = (N.ptr(W), N.ptr(b), 300, N.ptr(target), N.ptr(nll), N.ptr(lse), N.ptr(top1), N.ptr(ws))
    # M == 0
    assert lib.tal_xent_rows_fwd(N.ptr(feat), 0, 64, 64, *args, ws.numel(), N.stream_handle()) == 0
    assert lib.tal_xent_lse_rows(N.ptr(feat), 0, 64, N.ptr(target), N.ptr(nll), N.ptr(lse), N.ptr(top1), N.stream_handle()) == 0
    # a short workspace, either form
    for form in (1, 2):
        with _Options(xent_form=form):
            assert lib.tal_xent_rows_fwd(N.ptr(feat), ref.M, 64, 64, *args, 64, N.stream_handle()) == -2
            assert b"workspace 64 <" in lib.tal_last_error()
            assert lib.tal_xent_rows_fwd(N.ptr(feat), ref.M, 64, 64, *args[:-1], None, ws.numel(), N.stream_handle()) == -2
    # null pointers, bad shapes
    assert lib.tal_xent_rows_fwd(N.ptr(feat), ref.M, 64, 64, N.ptr(W), N.ptr(b), 300, None, N.ptr(nll), None, None, N.ptr(ws), ws.numel(),
                                 N.stream_handle()) == -1 and b"null pointer" in lib.tal_last_error()
    assert lib.tal_xent_rows_fwd(N.ptr(feat), ref.M, 60, 64, *args, ws.numel(), N.stream_handle()) == -1 and b"bad shape" in lib.tal_last_error()
    # the fused form where the shape does not allow it is an error, not a fallback: another width, a pitch off the 16-byte grid, an
    # operand off it
    f32w, w32, b32, t32, _ = _to_dev(*R.build("random-31-127-32-pitch")[:4], None)
    with _Options(xent_form=2):
        assert lib.tal_xent_rows_fwd(N.ptr(f32w), 31, 48, 32, N.ptr(w32), N.ptr(b32), 127, N.ptr(t32), N.ptr(nll), None, None, N.ptr(ws), ws.numel(),
                                     N.stream_handle()) == -1 and b"fused form" in lib.tal_last_error()
        wide = torch.zeros(8, 66, device=dev())
        assert lib.tal_xent_rows_fwd(N.ptr(wide), 8, 66, 64, *args, ws.numel(), N.stream_handle()) == -1 and b"fused form" in lib.tal_last_error()
        assert lib.tal_xent_rows_fwd(C.c_void_p(feat.data_ptr() + 4), 8, 64, 64, *args, ws.numel(), N.stream_handle()) == -1
        with pytest.raises(NativeError, match="fused form"):
            ops.xent_rows(f32w[:, :32].contiguous(), w32, b32, t32)
    _unguard(0, nll, lse, top1)       # nothing was written by any of these
    # auto dispatch gives one of the two forms' results; a width the fused kernel does not take runs the generic form
    auto = xent_rows(feat, W, b, target, 0)
    assert any(all(np.array_equal(_bits(a), _bits(c)) for a, c in zip(auto, xent_rows(feat, W, b, target, f))) for f in (1, 2))
    out = ops.xent_rows(f32w[:, :32].contiguous().reshape(1, 31, 32), w32, b32, t32.reshape(1, 31), want_lse=True, want_top1=True)
    assert [tuple(o.shape) for o in out] == [(1, 31)] * 3 and out[2].dtype == torch.int32
    assert R.compare(R.build("random-31-127-32-pitch")[4], *[o[0].cpu().numpy() for o in out]) == []
    with pytest.raises(NativeError):
        ops.xent_rows(feat, W, b, target.to(torch.float32))


def test_three_calls_are_bit_identical():
    for name in R.REPEAT_CASES:
        feat_h, W_h, b_h, target_h, ref = R.build(name)
        feat, W, b, target = _to_dev(feat_h, W_h, b_h, target_h)
        for form in (1, 2):
            first = xent_rows(feat, W, b, target, form)
            assert R.compare(ref, *first) == [], (name, form)
            for _ in range(2):
                again = xent_rows(feat, W, b, target, form)
                for a, c in zip(first, again):
                    assert np.array_equal(_bits(a), _bits(c)), (name, form)


def test_generic_form_in_small_pieces():
    """The generic form takes as many rows at a time as its workspace holds: three rows' worth gives the bits of the full workspace
    (the rows do not interact), with the bytes behind it untouched."""
    from tal_asrd_amd import _native as N
    lib = N.lib()
    feat_h, W_h, b_h, target_h, ref = R.build("random-257-300-64")
    feat, W, b, target = _to_dev(feat_h, W_h, b_h, target_h)
    full = xent_rows(feat, W, b, target, 1)
    nll, lse, top1 = _guarded(ref.M)
    nws = 3 * 300 * 4 + 100
    ws = torch.full((nws + 256,), 0xAB, dtype=torch.uint8, device=dev())
    with _Options(xent_form=1):
        N.check(lib.tal_xent_rows_fwd(N.ptr(feat), ref.M, 64, 64, N.ptr(W), N.ptr(b), 300, N.ptr(target), N.ptr(nll), N.ptr(lse), N.ptr(top1),
                                      N.ptr(ws), nws, N.stream_handle()), "tal_xent_rows_fwd")
    out = _unguard(ref.M, nll, lse, top1)
    assert bool((ws[nws:] == 0xAB).all()), "bytes behind the workspace written"
    for a, c in zip(full, out):
        assert np.array_equal(_bits(a), _bits(c))
    # the sizes the library asks for: partials where it expects the fused form by shape, 64 MiB of logits at most otherwise
    assert lib.tal_xent_rows_workspace_bytes(8192, 16008, 64) < 8192 * 16008 * 4 // 100
    assert lib.tal_xent_rows_workspace_bytes(8192, 16008, 256) == (64 << 20) // (16008 * 4) * 16008 * 4
    with _Options(xent_form=1):
        assert lib.tal_xent_rows_workspace_bytes(8192, 16008, 64) == lib.tal_xent_rows_workspace_bytes(8192, 16008, 256)


@pytest.mark.parametrize("name", sorted(R.ROWS_CASES))
def test_xent_lse_rows(name):
    from tal_asrd_amd import _native as N, ops
    x_h, target_h, ref = R.build_rows(name)
    x, target = _to_dev(x_h, target_h)
    nll, lse, top1 = _guarded(ref.M)
    N.check(N.lib().tal_xent_lse_rows(N.ptr(x), ref.M, ref.N, N.ptr(target), N.ptr(nll), N.ptr(lse), N.ptr(top1), N.stream_handle()),
            "tal_xent_lse_rows")
    out = _unguard(ref.M, nll, lse, top1)
    assert R.compare(ref, *out) == [], name
    # the wrapper, and NULL lse / top1
    n2 = ops.xent_lse_rows(x.reshape(1, ref.M, ref.N), target.reshape(1, ref.M))
    assert tuple(n2.shape) == (1, ref.M) and np.array_equal(_bits(n2[0].cpu().numpy()), _bits(out[0])), name


# ------------------------------------------------------------------ the LM head entry point and the models
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


def _tokens(seed, B, U, V):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, V, size=(B, U)).astype(np.int64)).to(dev())


def _nll64(logits, target):
    """float64 log-softmax + gather of materialised logits; 0 where the target is negative."""
    lp = torch.log_softmax(logits.double(), dim=-1)
    t = target.clamp(min=0)
    return torch.where(target >= 0, -lp.gather(-1, t.unsqueeze(-1)).squeeze(-1), torch.zeros_like(lp[..., 0])).cpu().numpy()


def _lm_ref(m, h, target):
    """The float64 model of the tied LM head on the hidden rows h [M, D], with the two-stage bound: the projected row t carries
    gamma_{D+2} |h| |P|, which the head multiplies by |emb| on top of its own gamma_{E0+2} |t| |emb|."""
    h64 = h.double().cpu().numpy()
    emb = m.embedding.weight.detach().double().cpu().numpy()
    if m.embed_size:
        P = m.embedding_proj.weight.detach().double().cpu().numpy()           # [D, E0]: t = h . P
        t = h64 @ P
        dt = R.gamma(P.shape[0] + 2) * (np.abs(h64) @ np.abs(P))
    else:
        t, dt = h64, np.zeros_like(h64)
    B = R.gamma(emb.shape[1] + 2) * (np.abs(t) @ np.abs(emb).T) + (1 + 1e-6) * (dt @ np.abs(emb).T)
    return R.Ref(t @ emb.T, B, target.cpu().numpy(), False)


def lm_xent(m, h, M, ldh, target, form, grid=0):
    """tal_lm_xent_fwd through the C ABI on M rows of pitch ldh, guard rows and guard bytes as xent_rows."""
    from tal_asrd_amd import _native as N, decoder
    lib = N.lib()
    V, E0 = m.embedding.weight.shape
    D = h.shape[-1]
    pt = decoder._proj_t(m) if m.embed_size else None
    nll, lse, top1 = _guarded(M)
    with _Options(xent_form=form, xent_grid=grid):
        nws = lib.tal_lm_xent_workspace_bytes(M, D, E0, V)
        ws = torch.full((nws + 256,), 0xAB, dtype=torch.uint8, device=dev())
        N.check(lib.tal_lm_xent_fwd(C.c_void_p(h.data_ptr()), M, ldh, D, N.ptr(pt), E0, N.ptr(m.embedding.weight), V, N.ptr(target), N.ptr(nll),
                                    N.ptr(lse), N.ptr(top1), N.ptr(ws), nws, N.stream_handle()), "tal_lm_xent_fwd")
        short = lib.tal_lm_xent_fwd(C.c_void_p(h.data_ptr()), M, ldh, D, N.ptr(pt), E0, N.ptr(m.embedding.weight), V, N.ptr(target), N.ptr(nll),
                                    N.ptr(lse), N.ptr(top1), N.ptr(ws), 16, N.stream_handle())
    assert short == -2
    out = _unguard(M, nll, lse, top1)
    assert bool((ws[nws:] == 0xAB).all()), "bytes behind the workspace written"
    return out


@pytest.mark.parametrize("tag", ("2x_tok", "1x_e0"))
def test_lm_xent_against_lm_head(tag):
    """tal_lm_xent_fwd against lm_head + float64 log-softmax + gather on the same hidden states (E0 = 64, V = 16008: fused and generic;
    no projection, D = 256: generic), U = 7 and 64, and on the last position only through a pitched h."""
    from tal_asrd_amd import NativeError, decoder, synth
    m = _model(tag)
    V = m.embedding.weight.shape[0]
    audio = torch.from_numpy(synth.synth_audio_batch(2, 160000, 1234, lens=[160000, 120000])).to(dev())
    enc = m.encode(audio, torch.tensor([160000, 120000]))
    for U in (7, 64):
        y = _tokens(U, 2, U, V)
        target = _tokens(100 + U, 2, U, V)
        target[0, 1], target[1, U - 1] = -1, V - 1
        h = decoder._run_stack(m, m.decoder, y, enc["encoder_out"], enc["encoder_padding_mask"], True)
        logits = decoder.lm_head(m, h)
        want = _nll64(logits, target).reshape(-1)
        ref = _lm_ref(m, h.reshape(2 * U, -1), target.reshape(-1))
        assert ref.unclear_share <= R.UNCLEAR_CAP
        runs = [(1, 0)] + ([(2, 0), (2, 3)] if m.embed_size else [])
        for form, grid in runs:
            nll, lse, top1 = lm_xent(m, h, 2 * U, h.shape[-1], target, form, grid)
            assert R.compare(ref, nll, lse, top1) == [], (tag, U, form, grid)
            # lm_head's logits are within B of the model too: the two paths differ by at most twice the bound
            assert (np.abs(nll - want) <= 2 * (ref.Bt + ref.Bmax + (V + 64) * R.U)).all(), (tag, U, form, grid)
            assert np.array_equal(top1[ref.clear], logits.reshape(2 * U, V).argmax(-1).cpu().numpy()[ref.clear]), (tag, U, form, grid)
            # the last position only, through h's pitch of U rows: the same rows, the same bound
            last = target[:, U - 1].contiguous()
            n1, l1, t1 = lm_xent(m, h[:, U - 1], 2, U * h.shape[-1], last, form, grid)
            rl = _lm_ref(m, h[:, U - 1], last)
            assert R.compare(rl, n1, l1, t1) == [], (tag, U, form, grid)
            assert (np.abs(n1 - nll.reshape(2, U)[:, -1]) <= 2 * (rl.Bt + rl.Bmax + (V + 64) * R.U)).all()
        if not m.embed_size:
            with _Options(xent_form=2):
                with pytest.raises(NativeError, match="fused form"):
                    decoder.lm_xent(m, h, target)


def test_asr_model_score_against_decode():
    """ASRModel.score equals decode / decode_spk + float64 log-softmax + gather within 2 LOGIT_TOL: nll is 1-Lipschitz in each of lse
    and the target's logit, and the project's logit tolerance is 1e-3 (the two paths run the same kernels up to the head, so the
    difference measured on the MI355X is far smaller: 1.1e-6 for the LM head, 7.2e-6 for the speaker head)."""
    from tal_asrd_amd import decoder, synth
    m = _model("2x_spk")
    V, S = m.embedding.weight.shape[0], m.speaker_head[1].weight.shape[0]
    audio = torch.from_numpy(synth.synth_audio_batch(2, 160000, 1234, lens=[160000, 120000])).to(dev())
    enc = m.encode(audio, torch.tensor([160000, 120000]))
    U = 24
    y, target, spk = _tokens(1, 2, U, V), _tokens(2, 2, U, V), _tokens(3, 2, U, S)
    target[1, 20:], spk[1, 20:] = -1, -1
    r = m.score(y, target, enc, spk_target=spk, want_top1=True)
    lm_logits, spk_logits = m.decode(y, enc), m.decode_spk(y, enc)
    for what, nll, top1, logits, t in (("lm", r.lm_nll, r.lm_top1, lm_logits, target), ("spk", r.spk_nll, r.spk_top1, spk_logits, spk)):
        assert tuple(nll.shape) == (2, U) and top1.dtype == torch.int32
        err = np.abs(nll.cpu().numpy() - _nll64(logits, t)).max()
        print("ASRModel.score %s: max |nll - (decode + float64 log-softmax + gather)| = %.3e" % (what, err))
        assert err <= 2 * LOGIT_TOL, what
        assert (nll[1, 20:] == 0).all(), what
        top2 = torch.topk(logits, 2, dim=-1).values
        sure = ((top2[..., 0] - top2[..., 1]) > 2 * LOGIT_TOL).cpu().numpy()
        assert sure.mean() > 0.9
        assert np.array_equal(top1.cpu().numpy()[sure], logits.argmax(-1).cpu().numpy()[sure]), what
    plain = m.score(y, target, enc)
    assert plain.spk_nll is None and plain.lm_top1 is None and torch.equal(plain.lm_nll, r.lm_nll)
    # targets are checked on the host: one past the vocabulary raises instead of scoring +inf silently
    bad = target.clone()
    bad[0, 3] = V
    with pytest.raises(ValueError):
        decoder.asr_score(m, y, bad, enc)
    with pytest.raises(ValueError):
        decoder.asr_score_spk(m, y, torch.full_like(spk, S), enc)
    with pytest.raises(IndexError):
        decoder.asr_score(m, bad, target, enc)          # (y_prev goes through _embed's own check)


class _Tok:
    eos_token_id, bos_token_id, pad_token_id = 1, 0, 2

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


@pytest.mark.parametrize("cfg", ("a", "b"))
def test_validation_step_and_score_against_the_reference(cfg):
    """System.validation_step / System.score against the reference's own System.training_step in eval mode (tests/golden/asr_score.npz,
    recorded by make_golden_score.py): a = speaker ids as vocabulary tokens, spk_weight 0, one id above the unknown-speaker clamp;
    b = speaker head, spk_weight 0.5.  The three losses within 2 LOGIT_TOL = 2e-3 (a mean of nlls, each 1-Lipschitz in lse and in the
    target's logit); the per-position nlls within the same, the per-sequence sums within that times the sequence's count.
    Measured on the MI355X: all three losses of both configurations equal the reference's to the last printed digit (|diff| below
    1e-6 of values 10.6, 63.1, 41.7); per position the lm nll is within 2.5e-6 (a), 2.1e-6 (b), the speaker nll within 5.0e-5 (values
    of 30 to 100) -- a margin of 40x to the tolerance at the least."""
    from tal_asrd_amd import synth
    from tal_asrd_amd.system import System
    g = golden("asr_score")
    V0, S = int(g["vocab_size"]), int(g["num_speakers"])
    m = _model("2x_tok" if cfg == "a" else "2x_spk")
    lens = [int(x) for x in g["audio_lens"]]
    audio = torch.from_numpy(synth.synth_audio_batch(2, lens[0], int(g["audio_seed"]), lens=lens)).to(dev())
    y, y_mask, spk_ids = (torch.from_numpy(g[k]).to(dev()) for k in ("y_" + cfg, "y_mask", "spk_ids"))
    system = System(m, spk_weight=float(g["spk_weight_" + cfg]), tokenizer=_Tok(V0))
    batch = (audio, torch.tensor(lens), y, y_mask, spk_ids)
    out = system.validation_step(batch, 0)
    assert sorted(out) == ["val_lm_loss", "val_loss", "val_spk_loss"] and all(v.is_cuda and v.dim() == 0 for v in out.values())
    for k in ("lm_loss", "spk_loss", "loss"):
        got, want = float(out["val_" + k]), float(g[k + "_" + cfg])
        print("config %s val_%s: %.6f vs the reference's %.6f (|diff| %.3e)" % (cfg, k, got, want, abs(got - want)))
    for k in ("lm_loss", "spk_loss", "loss"):
        assert abs(float(out["val_" + k]) - float(g[k + "_" + cfg])) <= 2 * LOGIT_TOL, k
    if cfg == "a":
        bound = V0 + S - 1
        assert int(y.max()) > bound                      # the clamp is exercised: without it the id is refused on the host
        with pytest.raises((IndexError, ValueError)):
            system.score(audio, torch.tensor(lens), y, y_mask)
        y = torch.clamp(y, max=bound)
    s = system.score(audio, torch.tensor(lens), y, y_mask, spk_ids)
    keep = g["y_mask"][:, 1:]
    np.testing.assert_array_equal(s.count.cpu().numpy(), keep.sum(axis=1))
    pairs = [("lm", s.lm_nll, s.lm_sum, g["lm_nll_" + cfg])]
    if cfg == "b":
        pairs.append(("spk", s.spk_nll, s.spk_sum, g["spk_nll_b"]))
    else:
        assert s.spk_nll is None and s.spk_sum is None
    for what, nll, total, want in pairs:
        nll, total = nll.cpu().numpy(), total.cpu().numpy()
        assert (nll[~keep] == 0).all(), what
        err = np.abs(nll - want)[keep].max()
        print("config %s %s: max per-position |nll - reference| = %.3e" % (cfg, what, err))
        assert err <= 2 * LOGIT_TOL, what
        np.testing.assert_allclose(total, np.where(keep, want, 0.0).sum(axis=1), rtol=0, atol=2 * LOGIT_TOL * keep.sum(axis=1).max())
    # validation_end of two steps is their mean
    mask2 = y_mask.clone()
    mask2[:, 12:] = False
    out2 = system.validation_step((audio, torch.tensor(lens), torch.from_numpy(g["y_" + cfg]).to(dev()), mask2, spk_ids), 1)
    end = system.validation_end([out, out2])
    for k in out:
        assert abs(float(end[k]) - 0.5 * (float(out[k]) + float(out2[k]))) <= 1e-6 * max(1.0, abs(float(out[k]))), k
        assert end["log"][k] is end[k]
    assert abs(float(out2["val_lm_loss"]) - float(out["val_lm_loss"])) > 1e-3      # (the second step is another batch)
