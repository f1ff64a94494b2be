"""ops.speaker_turns / ops.segment_mean / SDModel.speaker_turns on the GPU (csrc/turns.hip) against tests/_turns_ref.py.
Every integer output must EQUAL the host model; the turn embeddings and segment_mean lie within the derived first-order bound
of the float64 mean (|y - y64| <= n 2^-24 mean|x| + 2^-24 |y64|, _turns_ref.segment_mean_bound) and are bit-identical call
after call and whatever other ranges share the call.

Two test items: the suite is long already, so the cases run as loops inside them, every assertion naming its case; the list of
integer cases is tests/_turns_ref.cases, which tests/test_turns_ref_cpu.py walks case by case on the host."""
import numpy as np
import pytest
import torch

from tests import _turns_ref as R

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _tile():
    from tal_asrd_amd import ops
    return ops.speaker_turns_tile()


def _check(res, ref, what):
    for f in ("offsets", "start", "end", "label", "purity", "frame_labels"):
        got = getattr(res, f).cpu().numpy()
        want = getattr(ref, f)
        assert got.dtype == want.dtype, (what, f, got.dtype)
        np.testing.assert_array_equal(got, want, err_msg="%s: %s" % (what, f))


def _run(ids, num_ids, off, w, m, feat=None):
    from tal_asrd_amd import ops
    return ops.speaker_turns(torch.from_numpy(np.asarray(ids, np.int32)).to(dev()), num_ids, offsets=off, smooth=w, min_frames=m,
                             feat=feat, want_frames=True)


def _cases():
    # (collected without the library: the tile length is checked against the library in the first test)
    return R.cases(256)


def _tile_is_what_the_cases_were_built_for():
    T, wmax = _tile()
    assert (T, wmax) == (256, 31)


def _integer_outputs_equal_the_model(case):
    name, ids, num_ids, off, w, m = case
    res = _run(ids, num_ids, off, w, m)
    _check(res, R.speaker_turns(ids, num_ids, off, w, m), name)
    assert res.embed is None and res.num_turns == int(res.offsets[-1])


def _without_frames_and_reshaped_ids():
    from tal_asrd_amd import ops
    ids = R.sticky_chain(4 * 300, 3, 0.8, 5)
    off = [0, 300, 600, 900, 1200]
    res = ops.speaker_turns(torch.from_numpy(ids).to(dev()).reshape(4, 300), 3, offsets=np.asarray(off), smooth=2, min_frames=4)
    ref = R.speaker_turns(ids, 3, off, 2, 4)
    assert res.frame_labels is None
    for f in ("offsets", "start", "end", "label", "purity"):
        np.testing.assert_array_equal(getattr(res, f).cpu().numpy(), getattr(ref, f))


def _empty_calls():
    res = _run(np.zeros(0, np.int32), 3, None, 2, 2)
    assert res.num_turns == 0 and res.offsets.tolist() == [0, 0] and res.frame_labels.numel() == 0
    res = _run(np.zeros(0, np.int32), 3, [0, 0, 0], 2, 2, feat=torch.zeros(0, 8, device=dev()))
    assert res.num_turns == 0 and res.offsets.tolist() == [0, 0, 0] and tuple(res.embed.shape) == (0, 8)


def _out_of_range_id_raises_and_the_next_call_is_right(bad):
    from tal_asrd_amd import NativeError
    T, _ = _tile()
    ids = R.sticky_chain(2 * T + 3, 40, 0.8, 3)
    broken = ids.copy()
    broken[T + 1] = bad
    with pytest.raises(NativeError, match="outside"):
        _run(broken, 40, None, 3, 2)
    _check(_run(ids, 40, None, 3, 2), R.speaker_turns(ids, 40, None, 3, 2), "after a refused call")


def _bad_arguments_raise():
    from tal_asrd_amd import NativeError, ops
    ids = torch.zeros(16, dtype=torch.int32, device=dev())
    with pytest.raises(NativeError):
        ops.speaker_turns(ids, 4, smooth=32)
    with pytest.raises(NativeError):
        ops.speaker_turns(ids, 4, smooth=-1)
    with pytest.raises(NativeError):
        ops.speaker_turns(ids, 4, min_frames=0)
    with pytest.raises(NativeError):
        ops.speaker_turns(ids, 0)
    with pytest.raises(NativeError):
        ops.speaker_turns(ids, 4, offsets=[0, 9, 8, 16])
    with pytest.raises(NativeError):
        ops.speaker_turns(ids, 4, offsets=[0, 15])
    with pytest.raises(NativeError):
        ops.speaker_turns(ids.to(torch.int64), 4)
    with pytest.raises(NativeError):
        ops.speaker_turns(ids.cpu(), 4)
    with pytest.raises(NativeError):
        ops.speaker_turns(ids, 4, feat=torch.zeros(16, 8))                     # CPU features
    with pytest.raises(NativeError):
        ops.speaker_turns(ids, 4, feat=torch.zeros(16, 6, device=dev()))       # E % 4
    with pytest.raises(NativeError):
        ops.segment_mean(torch.zeros(16, 8), [[0, 4]])
    with pytest.raises(NativeError):
        ops.segment_mean(torch.zeros(16, 6, device=dev()), [[0, 4]])
    with pytest.raises(NativeError, match="range"):
        ops.segment_mean(torch.zeros(16, 8, device=dev()), [[0, 17]])
    with pytest.raises(NativeError, match="range"):
        ops.segment_mean(torch.zeros(16, 8, device=dev()), [[5, 4]])
    # the C entry refuses what the wrapper would: nothing is launched (rc = TAL_EINVAL)
    lib = ops.N.lib()
    off = np.array([0, 16], np.int64)
    rc = lib.tal_speaker_turns_fwd(ops.N.ptr(ids), off.ctypes.data, ops.N.ptr(ids), 1, 4, 32, 1, None, None, None, None, None, None,
                                   ops.N.ptr(ids), ops.N.ptr(ids), None, 0, None)
    assert rc == -1 and b"smooth" in lib.tal_last_error()


# ---------------------------------------------------------------- segment mean
def _seg_data():
    """feat [5300, E] for E = 4 and 128: O(1e-3) rows with rows of 1e4 among them, and the ranges under test"""
    from tal_asrd_amd import ops
    Cn = ops.SEGMENT_MEAN_CHUNK
    rng = np.random.RandomState(21)
    feats = {}
    for E in (4, 128):
        x = (rng.randn(5300, E) * 1e-3).astype(np.float32)
        x[[0, 77, 200, 1234, 5000]] = 1e4
        x[300] = -1e4
        feats[E] = x
    ranges = [(77, 78), (10, 10 + Cn - 1), (150, 150 + Cn), (190, 190 + Cn + 1), (100, 5100), (0, 5300), (40, 40), (76, 79)]
    return Cn, feats, ranges


def _segment_mean_bound_and_bits(seg_data, E):
    from tal_asrd_amd import ops
    Cn, feats, ranges = seg_data
    x = feats[E]
    xd = torch.from_numpy(x).to(dev())
    y64 = R.segment_mean64(x, ranges)
    bound = R.segment_mean_bound(x, ranges, y64)
    y = ops.segment_mean(xd, ranges)
    assert y.dtype == torch.float32 and tuple(y.shape) == (len(ranges), E)
    err = np.abs(y.cpu().numpy().astype(np.float64) - y64)
    print("E=%d max err / bound = %.3f" % (E, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all(), float((err - bound).max())
    assert (y[6] == 0).all()                                       # the empty range
    assert torch.equal(y[0].cpu(), torch.from_numpy(x[77]))         # one row: exact
    # call after call, host ranges or device ranges
    assert torch.equal(ops.segment_mean(xd, ranges), y)
    assert torch.equal(ops.segment_mean(xd, torch.tensor(ranges, device=dev())), y)
    # alone or among 100 others (before, behind, overlapping, in another order)
    rng = np.random.RandomState(5)
    for g, r in enumerate(ranges):
        assert torch.equal(ops.segment_mean(xd, [r])[0], y[g]), g
    others = []
    for _ in range(100):
        a = int(rng.randint(0, 5300))
        others.append((a, int(rng.randint(a, min(5300, a + 700) + 1))))
    mixed = others[:37] + [ranges[4]] + others[37:80] + [ranges[3], ranges[1]] + others[80:]
    ym = ops.segment_mean(xd, mixed)
    assert torch.equal(ym[37], y[4]) and torch.equal(ym[81], y[3]) and torch.equal(ym[82], y[1])
    ob = R.segment_mean_bound(x, others, R.segment_mean64(x, others))
    got = torch.cat((ym[:37], ym[38:81], ym[83:])).cpu().numpy().astype(np.float64)
    assert (np.abs(got - R.segment_mean64(x, others)) <= ob).all()


def _segment_mean_wide_and_odd_widths():
    from tal_asrd_amd import ops
    rng = np.random.RandomState(9)
    for E in (12, 1024):
        x = rng.randn(700, E).astype(np.float32)
        ranges = [(0, 700), (5, 6), (100, 357)]
        y64 = R.segment_mean64(x, ranges)
        y = ops.segment_mean(torch.from_numpy(x).to(dev()), ranges).cpu().numpy().astype(np.float64)
        assert (np.abs(y - y64) <= R.segment_mean_bound(x, ranges, y64)).all(), E


def _turn_embeddings(seg_data):
    """embed of speaker_turns = the segment mean of the turns' rows: within the bound, and the same bits as segment_mean"""
    from tal_asrd_amd import ops
    _, feats, _ = seg_data
    T, _ = _tile()
    lens = [1, T + 3, 0, 2, T - 1, 0, 2000]
    off = np.concatenate([[0], np.cumsum(lens)])
    n = int(off[-1])
    ids = R.sticky_chain(n, 3, 0.9, 31)
    ids[off[6] + 100:] = 2                     # a long monologue: many chunks in one range
    x = feats[128][:n]
    xd = torch.from_numpy(x).to(dev())
    res = _run(ids, 3, off, 3, 5, feat=xd)
    ref = R.speaker_turns(ids, 3, off, 3, 5)
    _check(res, ref, "with features")
    ranges = []
    for b in range(len(lens)):
        for k in range(int(ref.offsets[b]), int(ref.offsets[b + 1])):
            ranges.append((int(off[b]) + int(ref.start[k]), int(off[b]) + int(ref.end[k])))
    assert max(b - a for a, b in ranges) > 1500
    y64 = R.segment_mean64(x, ranges)
    got = res.embed.cpu().numpy().astype(np.float64)
    assert got.shape == y64.shape
    assert (np.abs(got - y64) <= R.segment_mean_bound(x, ranges, y64)).all()
    assert torch.equal(res.embed, ops.segment_mean(xd, ranges))
    assert torch.equal(_run(ids, 3, off, 3, 5, feat=xd.reshape(1, n, 128)).embed, res.embed)


# ---------------------------------------------------------------- the model entry point
def _sd_model(sd_weights):
    from tal_asrd_amd import SDModel
    model = SDModel()
    own = model.state_dict()
    for k, v in sd_weights.items():
        assert k in own, k
        own[k] = torch.from_numpy(np.array(v, copy=True))
    model.load_state_dict(own)
    return model.to(dev())


def _sdmodel_speaker_turns(sd_model):
    from tal_asrd_amd import rttm, synth
    audio = torch.from_numpy(synth.synth_audio_batch(1, 30 * 16000, 4321)).to(dev())
    feat0, ids0 = sd_model.speaker_ids(audio)
    res = sd_model.speaker_turns(audio)
    feat1, ids1 = sd_model.speaker_ids(audio)
    assert torch.equal(feat0, feat1) and torch.equal(ids0, ids1)
    ids = ids0.cpu().numpy().reshape(-1)
    x = feat0.cpu().numpy().reshape(len(ids), -1)
    num_ids = sd_model.spk_logit_proj.weight.shape[0]
    ref = R.speaker_turns(ids, num_ids, None, 6, 13)
    _check(res, ref, "SDModel.speaker_turns")
    ranges = list(zip(ref.start.tolist(), ref.end.tolist()))
    y64 = R.segment_mean64(x, ranges)
    got = res.embed.cpu().numpy().astype(np.float64)
    assert got.shape == y64.shape and (np.abs(got - y64) <= R.segment_mean_bound(x, ranges, y64)).all()
    # other settings, no embeddings, the log-mel form; text out
    res2 = sd_model.speaker_turns(audio, smooth=0, min_frames=1, want_embeds=False)
    _check(res2, R.speaker_turns(ids, num_ids, None, 0, 1), "smooth=0")
    assert res2.embed is None
    mel, mean = sd_model.logmelspec.forward_unsubtracted(audio)
    res3 = sd_model.speaker_turns_from_logmel(mel, mean)
    _check(res3, ref, "from_logmel")
    assert torch.equal(res3.embed, res.embed)
    secs = rttm.turns_to_seconds(res, 0)
    assert len(secs) == res.num_turns and secs[0][0] == 0.0 and abs(secs[-1][1] - len(ids) * 0.08) < 1e-9


def _sdmodel_speaker_turns_batch(sd_model):
    """every row of a batched call is one item"""
    from tal_asrd_amd import synth
    audio = torch.from_numpy(synth.synth_audio_batch(3, 5 * 16000, 99)).to(dev())
    feat, ids = sd_model.speaker_ids(audio)
    res = sd_model.speaker_turns(audio, smooth=2, min_frames=3)
    frames = ids.shape[-1]
    ref = R.speaker_turns(ids.cpu().numpy().reshape(-1), sd_model.spk_logit_proj.weight.shape[0], [0, frames, 2 * frames, 3 * frames], 2, 3)
    _check(res, ref, "batched")
    assert tuple(res.embed.shape) == (res.num_turns, feat.shape[-1])


# ---------------------------------------------------------------- the two test items
def test_speaker_turns_integer_outputs_and_refusals():
    """every integer case of _turns_ref.cases (lengths round the tile and the window, ragged batches with empty items, w x m, the ends
    of the id range, one turn across tiles, N turns, hand-written ties, the step-c cases, sticky random chains), calls without frame
    labels, empty calls, ids of -1 and of num_ids (NativeError, and the next call is right), smooth = 32 and the other refusals,
    CPU tensors"""
    _tile_is_what_the_cases_were_built_for()
    for case in _cases():
        _integer_outputs_equal_the_model(case)
    _without_frames_and_reshaped_ids()
    _empty_calls()
    for bad in (-1, 40):
        _out_of_range_id_raises_and_the_next_call_is_right(bad)
    _bad_arguments_raise()


def test_segment_mean_turn_embeddings_and_sdmodel(sd_weights):
    """segment_mean (range lengths 1, chunk - 1, chunk, chunk + 1, 5,000 and more; E = 4, 128, 12, 1024; rows of 1e4 next to rows of
    1e-3): the bound against float64, the same bits call after call and alone or among 100 other ranges; the turn embeddings of
    speaker_turns; SDModel.speaker_turns on a 30 s clip and on a batch"""
    data = _seg_data()
    for E in (4, 128):
        _segment_mean_bound_and_bits(data, E)
    _segment_mean_wide_and_odd_widths()
    _turn_embeddings(data)
    model = _sd_model(sd_weights)
    _sdmodel_speaker_turns(model)
    _sdmodel_speaker_turns_batch(model)
