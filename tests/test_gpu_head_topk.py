"""Per-row top-k speaker posteriors without the logits (csrc/head_topk.hip: tal_spk_topk_fwd, tal_topk_lse_rows) against the float64
model of tests/_head_topk_ref.py: both forms (generic = dense layer + row kernel, fused = A-stationary MFMA kernel with running
top-k and online log-sum-exp), the fused form at launch sizes that put the boundaries between workgroups inside a row block, guard
rows behind every output, masked speakers, repeatability, and SDModel.speaker_topk on the 30-second fixture."""
import numpy as np
import pytest
import torch

from tests import _head_topk_ref as R
from tests.conftest import golden, has_gpu

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


def _guarded(M, k):
    ids = torch.full((M + GUARD, k), ID_GUARD, dtype=torch.int32, device=dev())
    logp = torch.full((M + GUARD, k), F_GUARD, dtype=torch.float32, device=dev())
    lse = torch.full((M + GUARD,), F_GUARD, dtype=torch.float32, device=dev())
    return ids, logp, lse


def _unguard(M, ids, logp, lse):
    torch.cuda.synchronize()
    assert bool((ids[M:] == ID_GUARD).all()) and bool((logp[M:] == F_GUARD).all()) and bool((lse[M:] == F_GUARD).all()), "guard rows written"
    return ids[:M].cpu().numpy(), logp[:M].cpu().numpy(), lse[:M].cpu().numpy()


def spk_topk(feat, W, b, k, form, grid=0):
    """tal_spk_topk_fwd through the C ABI with guard rows behind ids / logp / lse and guard bytes behind the workspace."""
    from tal_asrd_amd import _native as N
    lib = N.lib()
    M, E = feat.shape
    S = W.shape[0]
    ids, logp, lse = _guarded(M, k)
    with _Options(head_topk_form=form, head_topk_grid=grid):
        nws = lib.tal_spk_topk_workspace_bytes(M, S, E, k)
        ws = torch.full((nws + 256,), 0xAB, dtype=torch.uint8, device=dev())
        N.check(lib.tal_spk_topk_fwd(N.ptr(feat), M, E, N.ptr(W), N.ptr(b), S, k, N.ptr(ids), N.ptr(logp), N.ptr(lse), N.ptr(ws), nws,
                                     N.stream_handle()), "tal_spk_topk_fwd")
    out = _unguard(M, ids, logp, lse)
    assert bool((ws[nws:] == 0xAB).all()), "bytes behind the workspace written"
    return out


def _to_dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev()) for a in arrays]


def _runs(feat, W, b, k):
    yield "generic", spk_topk(feat, W, b, k, 1)
    for g in GRIDS:
        yield "fused grid %d" % g, spk_topk(feat, W, b, k, 2, g)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_both_forms_against_the_model(name):
    from tal_asrd_amd import ops
    feat_h, W_h, b_h, ref = R.build(name)
    feat, W, b = _to_dev(feat_h, W_h, b_h)
    k = ref.k
    logits = ops.linear(feat, W, b).cpu().numpy().astype(np.float64)          # the materialised logits (dense layer)
    am = np.argmax(logits, axis=1)                                            # (first maximum, as torch.argmax)
    must = np.ones(ref.M, bool) if ref.exact_valued else ref.clear
    results = {}
    for what, (ids, logp, lse) in _runs(feat, W, b, k):
        assert R.compare(ref, ids, logp, lse) == [], (name, what)
        np.testing.assert_array_equal(ids[must, 0], am[must], err_msg="%s %s: ids[:, 0] vs arg-max of the logits" % (name, what))
        # logp + lse gives the logits back: within B of the dense layer's (one rounding in logp = z - lse on top)
        zg = np.take_along_axis(logits, ids.astype(np.int64), axis=1)
        back = logp.astype(np.float64) + lse.astype(np.float64)[:, None]
        fin = np.isfinite(zg)
        bound = np.take_along_axis(ref.B, ids.astype(np.int64), axis=1) + 2 * R.U * (np.abs(zg) + np.abs(lse)[:, None])
        with np.errstate(invalid="ignore"):
            assert np.all(np.where(fin, np.abs(back - zg) <= bound, back == zg)), (name, what)
        results[what] = (ids, logp, lse)
    # the two forms agree: same ids wherever rounding cannot reorder (both passed `compare` against the same model above)
    gi = results["generic"][0]
    for what, (ids, _, _) in results.items():
        np.testing.assert_array_equal(ids[must], gi[must], err_msg="%s: %s vs generic" % (name, what))
    if k == 8:
        # k = 1 is column 0 of k = 8, bit for bit, in each form
        for form, what in ((1, "generic"), (2, "fused grid 0")):
            i1, p1, l1 = spk_topk(feat, W, b, 1, form)
            i8, p8, l8 = results[what]
            assert np.array_equal(i1[:, 0], i8[:, 0]) and np.array_equal(p1[:, 0].view(np.int32), p8[:, 0].view(np.int32)), (name, what)
            assert np.array_equal(l1.view(np.int32), l8.view(np.int32)), (name, what)


def test_masked_speakers_follow_the_rule():
    """All but three columns -inf at k = 8: the three finite columns by value, then -inf columns by ascending index with logp = -inf;
    lse is that of the three."""
    feat_h, W_h, b_h, ref = R.build("masked-33-300-8-three")
    feat, W, b = _to_dev(feat_h, W_h, b_h)
    finite = sorted(R.CASES["masked-33-300-8-three"]["finite"])
    rest = [c for c in range(300) if c not in finite][:5]
    for what, (ids, logp, lse) in _runs(feat, W, b, 8):
        assert all(sorted(r[:3]) == finite and r[3:] == rest for r in ids.tolist()), what
        assert np.isfinite(logp[:, :3]).all() and (logp[:, 3:] == -np.inf).all(), what
        z3 = ref.z[:, finite]
        want = np.log(np.exp(z3 - z3.max(1, keepdims=True)).sum(1)) + z3.max(1)
        assert np.all(np.abs(lse - want) <= ref.Bmax + (300 + 64) * R.U), what
    # one finite column: its logp is 0
    feat_h, W_h, b_h, ref = R.build("masked-129-6008-4-one")
    for what, (ids, logp, lse) in _runs(*_to_dev(feat_h, W_h, b_h), 4):
        assert (ids == np.array([5999, 0, 1, 2])).all() and (np.abs(logp[:, 0]) <= 1e-6).all() and (logp[:, 1:] == -np.inf).all(), what


def test_no_bias_means_zeros():
    feat_h, W_h, _, _ = R.build("random-129-300-8")
    ref = R.linear_ref(feat_h, W_h, None, 8)
    feat, W = _to_dev(feat_h, W_h)
    assert ref.unclear_share <= R.UNCLEAR_CAP
    for what, (ids, logp, lse) in _runs(feat, W, None, 8):
        assert R.compare(ref, ids, logp, lse) == [], what


def test_three_calls_are_bit_identical():
    feat_h, W_h, b_h, ref = R.build_repeat()
    feat, W, b = _to_dev(feat_h, W_h, b_h)
    for form in (1, 2):
        first = spk_topk(feat, W, b, ref.k, form)
        assert R.compare(ref, *first) == [], form
        for _ in range(2):
            again = spk_topk(feat, W, b, ref.k, form)
            for a, c in zip(first, again):
                assert np.array_equal(a.view(np.int32), c.view(np.int32)), form


def test_dispatch_by_shape_and_other_widths():
    """Auto dispatch gives one of the two forms' results at either side of its threshold; a feature width the fused kernel does not
    take runs the generic form under auto and is an error, not a fallback, when the fused form is demanded."""
    from tal_asrd_amd import NativeError, ops
    feat_h, W_h, b_h, ref = R.build("random-300-6008-8")
    feat, W, b = _to_dev(feat_h, W_h, b_h)
    auto = spk_topk(feat, W, b, 8, 0)
    assert any(all(np.array_equal(a.view(np.int32), c.view(np.int32)) for a, c in zip(auto, spk_topk(feat, W, b, 8, f))) for f in (1, 2))
    feat_h, W_h, b_h, ref = R.build_repeat()
    feat, W, b = _to_dev(feat_h, W_h, b_h)
    auto = spk_topk(feat, W, b, 8, 0)
    assert any(all(np.array_equal(a.view(np.int32), c.view(np.int32)) for a, c in zip(auto, spk_topk(feat, W, b, 8, f))) for f in (1, 2))
    g = torch.Generator().manual_seed(64)
    f64, w64, b64 = torch.randn(50, 64, generator=g), torch.randn(300, 64, generator=g) / 8, torch.randn(300, generator=g)
    ref = R.linear_ref(f64.numpy(), w64.numpy(), b64.numpy(), 4)
    ids, logp, lse = ops.spk_topk(f64.to(dev()), w64.to(dev()), b64.to(dev()), 4)
    assert ids.dtype == torch.int32 and ids.shape == (50, 4) and logp.shape == (50, 4) and lse.shape == (50,)
    assert R.compare(ref, ids.cpu().numpy(), logp.cpu().numpy(), lse.cpu().numpy()) == []
    with _Options(head_topk_form=2):
        with pytest.raises(NativeError, match="fused form"):
            ops.spk_topk(f64.to(dev()), w64.to(dev()), b64.to(dev()), 4)
    with pytest.raises(NativeError):
        ops.spk_topk(f64.to(dev()), w64.to(dev()), b64.to(dev()), 17)


def test_a_small_workspace_is_refused():
    from tal_asrd_amd import _native as N
    lib = N.lib()
    feat, W, b = _to_dev(*R.build("random-129-300-8")[:3])
    ids, logp, lse = _guarded(129, 8)
    for form in (1, 2):
        with _Options(head_topk_form=form):
            need = lib.tal_spk_topk_workspace_bytes(129, 300, 128, 8)
            ws = torch.empty(need, dtype=torch.uint8, device=dev())
            rc = lib.tal_spk_topk_fwd(N.ptr(feat), 129, 128, N.ptr(W), N.ptr(b), 300, 8, N.ptr(ids), N.ptr(logp), N.ptr(lse), N.ptr(ws), 64,
                                      N.stream_handle())
            assert rc == -2 and b"workspace 64 <" in lib.tal_last_error()
    _unguard(0, ids, logp, lse)       # nothing was written


@pytest.mark.parametrize("name", sorted(R.ROWS_CASES))
def test_topk_lse_rows(name):
    from tal_asrd_amd import _native as N
    x_h, ref = R.build_rows(name)
    x, = _to_dev(x_h)
    ids, logp, lse = _guarded(ref.M, ref.k)
    N.check(N.lib().tal_topk_lse_rows(N.ptr(x), ref.M, ref.S, ref.k, N.ptr(ids), N.ptr(logp), N.ptr(lse), N.stream_handle()), "tal_topk_lse_rows")
    assert R.compare(ref, *_unguard(ref.M, ids, logp, lse)) == [], name


def test_topk_lse_rows_wrapper_and_null_lse():
    from tal_asrd_amd import _native as N, ops
    x_h, ref = R.build_rows("random-6008-8")
    x, = _to_dev(x_h)
    ids, logp, lse = ops.topk_lse_rows(x.reshape(1, ref.M, ref.S), ref.k)
    assert ids.shape == (1, ref.M, ref.k) and lse.shape == (1, ref.M)
    assert R.compare(ref, ids[0].cpu().numpy(), logp[0].cpu().numpy(), lse[0].cpu().numpy()) == []
    i2, p2, _ = _guarded(ref.M, ref.k)
    N.check(N.lib().tal_topk_lse_rows(N.ptr(x), ref.M, ref.S, ref.k, N.ptr(i2), N.ptr(p2), None, N.stream_handle()), "tal_topk_lse_rows")
    torch.cuda.synchronize()
    assert torch.equal(i2[:ref.M], ids[0]) and torch.equal(p2[:ref.M], logp[0])


# ------------------------------------------------------------------ end to end
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


def test_speaker_topk_on_the_30_second_fixture(sd_model):
    """SDModel.speaker_topk against the reference model's own logits (tests/golden/sd_30s_topk.npz, recorded by make_golden_topk.py):
    the arg-max column identical to the fixture's and to sd_30s's ids, logp and lse within 2 LOGIT_TOL (logit error plus log-sum-exp
    error, each bounded by the project's 1e-3), the further ids identical on the rows whose recorded gap exceeds 2 LOGIT_TOL; and the
    features are speaker_ids' features bit for bit."""
    from tal_asrd_amd import synth
    g, g0 = golden("sd_30s_topk"), golden("sd_30s")
    k = int(g["k_ids"])
    audio = torch.from_numpy(synth.synth_audio_batch(1, int(g["audio_len"]), int(g["audio_seed"]))).to(dev())
    feat, ids, logp, lse = sd_model.speaker_topk(audio, k=k)
    feat0, ids0 = sd_model.speaker_ids(audio)
    assert torch.equal(feat, feat0)
    assert ids.dtype == torch.int32 and ids.shape == ids0.shape + (k,) and logp.shape == ids.shape and lse.shape == ids0.shape
    ids, logp, lse = ids.cpu().numpy().reshape(-1, k), logp.cpu().numpy().reshape(-1, k), lse.cpu().numpy().reshape(-1)
    np.testing.assert_array_equal(ids[:, 0], g["ids"][:, 0])
    np.testing.assert_array_equal(ids[:, 0], g0["ids"].reshape(-1))
    np.testing.assert_array_equal(ids[:, 0], ids0.cpu().numpy().reshape(-1))
    sure = g["min_gap"] > 2 * LOGIT_TOL
    assert sure.mean() >= 0.9
    np.testing.assert_array_equal(ids[sure], g["ids"][sure, :k])
    np.testing.assert_allclose(lse, g["lse"], atol=2 * LOGIT_TOL, rtol=0)
    # (every row: sorting is 1-Lipschitz, so the values match position by position whichever of a close pair comes first)
    np.testing.assert_allclose(logp, g["logp"][:, :k], atol=2 * LOGIT_TOL, rtol=0)
    # the other entry point, and k = 1
    mel, mean = sd_model.logmelspec.forward_unsubtracted(audio)
    f1, i1, p1, l1 = sd_model.speaker_topk_from_logmel(mel, mean, k=1)
    assert torch.equal(f1, feat0) and np.array_equal(i1.cpu().numpy().reshape(-1), ids[:, 0])
