"""The device-resident beam search step by step on synthetic logits, no model (tal_beam_init_fwd / tal_beam_select_fwd /
tal_beam_advance_fwd / tal_beam_gather_spk_fwd, csrc/beam.hip).

Yardsticks: the selection of every step is held against the existing tal_log_softmax_rows + tal_beam_topk on the same logits
(values as fp32 bits, indices equal); all state after every step -- token matrix, scores, done, finish records, counters, the
pinned done word -- against the numpy model of the loop (tests/_beam_ref.py); gathered speaker histories bit-equal to the
model's index_select + cat form.

Logits are multiples of 0.5, so values tie inside a row; on odd steps every row of the step carries the same logits, so
candidates of different rows tie too (rows that tied at the step before have equal scores)."""
import numpy as np
import pytest
import torch

from tests._beam_ref import BeamRef
from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

SHAPES = {                       # (B, beam, V, L0, length)
    "b1": (1, 1, 257, 1, 12),
    "b2x3": (2, 3, 255, 1, 12),
    "b3x8": (3, 8, 1000, 2, 10),
    "b5x4": (5, 4, 4097, 1, 8),
    "model_vocab": (2, 3, 16008, 1, 6),
    "rows512": (64, 8, 300, 1, 6),
}
TERM = 1


def dev():
    return torch.device("cuda:0")


def _boost_rows(schedule, t, B, beam, length):
    """Rows whose terminate token is raised at step t.  'slots': row r on a schedule of its own; 'items': all rows of item b at
    step 1 + b % 4, the last item at step 4 -- every slot has finished after 5 steps; None: never."""
    R = B * beam
    if schedule == "slots":
        return [r for r in range(R) if t == 1 + (3 * r) % max(1, length - 2)]
    if schedule == "items":
        if beam == 1:
            return [b for b in range(B) if t == (4 if b == B - 1 else b % 4)]
        return [b * beam + j for b in range(B) for j in range(beam) if t == (4 if b == B - 1 else 1 + b % 4)]
    return []


def _step_inputs(seed, t, rows, V, terminate, boost, nl, ns):
    g = torch.Generator().manual_seed(seed * 1000 + t)
    x = torch.round(torch.randn(rows, V, generator=g) * 4) / 2
    if t % 2 == 1:
        x[:] = x[0].clone()
    if terminate is not None:
        x[:, terminate] = -60.0
        for r in boost:
            if r < rows:
                x[r, terminate] = 60.0
    bias = torch.round(torch.randn(rows, nl, generator=g) * 8) / 8 if nl else None
    spk = torch.randn(rows, ns, generator=g) if ns else None
    return x, bias, spk


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _check_state(sess, ref, calls):
    st = sess.state()
    assert st["step"] == ref.step and st["n_done"] == int(ref.done.sum())
    np.testing.assert_array_equal(st["tokens"], ref.tokens)
    np.testing.assert_array_equal(_bits(st["scores"]), _bits(ref.scores))
    np.testing.assert_array_equal(st["done"], ref.done)
    rec_step, rec_score, rows = ref.record_arrays()
    np.testing.assert_array_equal(st["rec_step"], rec_step)
    np.testing.assert_array_equal(_bits(st["rec_score"]), _bits(rec_score))
    for slot in range(ref.R):
        row = rows.get(slot, np.zeros(0, np.int64))
        np.testing.assert_array_equal(st["rec_tokens"][slot, :row.size], row)
        assert not st["rec_tokens"][slot, row.size:].any()
    # the pinned words (the copy above waited for the stream): slots done, advance calls so far
    assert sess.done_host.tolist() == [int(ref.done.sum()), calls]
    return st


def drive(shape, terminate=TERM, schedule="slots", nl=0, ns=0, seed=0, ws=None, check=True):
    """Run the whole search; -> (final state, [(values, indices) per step], gathered speaker histories or None)."""
    from tal_asrd_amd.decoder import log_softmax
    from tal_asrd_amd.system import _beam_topk, _BeamSession
    B, beam, V, L0, length = shape
    g = torch.Generator().manual_seed(seed)
    gen0 = torch.randint(2, V, (B, L0), generator=g)
    sess = _BeamSession(gen0.to(dev()), beam, length, V, ns, ws=ws)
    ref = BeamRef(gen0.numpy(), beam, V, terminate, ns)
    trace = []
    for t in range(length):
        cur = 1 if t == 0 and beam > 1 else beam
        rows = B * cur
        x, bias, spk = _step_inputs(seed, t, rows, V, terminate, _boost_rows(schedule, t, B, beam, length), nl, ns)
        xd = x.to(dev())
        bd = None if bias is None else bias.to(dev())
        sd = None if spk is None else spk.to(dev())
        sess.select(t, cur, xd, bd)
        v, i = (a.cpu().numpy().copy() for a in sess.selection())
        if check and not ref.stopped:
            lp = log_softmax(xd)
            if bd is not None:
                lp[:, :nl] += bd
            mask = ref.mask()
            wv, wi = _beam_topk(lp, torch.from_numpy(ref.scores[:rows].copy()).to(dev()),
                                None if mask is None else torch.from_numpy(mask.astype(np.uint8)).to(dev()), B, cur, beam)
            np.testing.assert_array_equal(i, wi.cpu().numpy(), err_msg="step %d" % t)
            np.testing.assert_array_equal(_bits(v), _bits(wv.cpu().numpy()), err_msg="step %d" % t)
        sess.advance(t, cur, terminate, sd)             # (enqueued whether or not the search is over: a frozen state stays)
        ref.advance(v, i, None if spk is None else spk.numpy())
        if check:
            _check_state(sess, ref, t + 1)
        trace.append((_bits(v).copy(), i))
    st = sess.state()
    hist = None
    if ns:
        pairs = [(r["slot"], r["step"]) for r in ref.records] + [(row, ref.step - 1) for row in range(ref.R)]
        hist = sess.gather_spk(pairs).numpy()
        if check:
            for k, r in enumerate(ref.records):
                np.testing.assert_array_equal(_bits(hist[k, :r["step"] + 1]), _bits(r["spk"]))
                assert not hist[k, r["step"] + 1:].any()
            np.testing.assert_array_equal(_bits(hist[len(ref.records):, :ref.step]), _bits(ref.spk_embeds))
    return st, trace, hist, ref, sess


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_step_matches_topk_and_the_loop_model(name):
    """Ties, a terminate token raised per slot on a schedule: selection bits and all state after every step."""
    st, _, _, ref, _ = drive(SHAPES[name], schedule="slots")
    assert ref.records and st["step"] == ref.step


@pytest.mark.parametrize("name", ["b1", "b2x3"])
def test_steps_enqueued_after_the_last_slot_finished_change_nothing(name):
    """Every slot finishes by step 5 of 12; the other 7 select / advance pairs are enqueued anyway: the state is the one after
    step 5 and the counter says so."""
    st, _, _, ref, sess = drive(SHAPES[name], schedule="items")
    assert ref.stopped and ref.step == 5 and st["step"] == 5 and st["n_done"] == ref.R
    assert st["tokens"].shape == (ref.R, SHAPES[name][3] + 5)
    assert sess.finished()


@pytest.mark.parametrize("name", ["b2x3", "b3x8"])
def test_without_a_terminate_token(name):
    st, _, _, ref, sess = drive(SHAPES[name], terminate=None, schedule=None)
    assert st["step"] == SHAPES[name][4] and not st["done"].any() and (st["rec_step"] == -1).all() and not sess.finished()


@pytest.mark.parametrize("name,nl", [("b2x3", 100), ("model_vocab", 10000), ("b1", 257)])
def test_with_a_bias_block(name, nl):
    """The LM's additive block on the first nl <= V columns: a separate rounding between the log-softmax and the score add."""
    kw = dict(terminate=None, schedule=None) if name == "b1" else {}      # (one row: its schedule would end the search after two steps)
    _, trace, _, _, _ = drive(SHAPES[name], nl=nl, **kw)
    _, plain, _, _, _ = drive(SHAPES[name], check=False, **kw)
    assert any((a[1] != b[1]).any() for a, b in zip(trace, plain))       # the block changes what is selected


@pytest.mark.parametrize("name,ns", [("b2x3", 7), ("b3x8", 6008), ("b1", 6008)])
def test_speaker_histories_follow_the_parent_rows(name, ns):
    _, _, hist, ref, _ = drive(SHAPES[name], ns=ns)
    assert hist is not None and ref.records


def test_same_call_twice_and_a_reused_workspace_give_the_same_bits():
    big, small = SHAPES["b3x8"], SHAPES["b2x3"]
    a = drive(small, ns=7, seed=3, check=False)
    b = drive(small, ns=7, seed=3, check=False)
    _, _, _, _, sess = drive(big, ns=7, seed=4, check=False)
    c = drive(small, ns=7, seed=3, ws=sess.ws, check=False)          # the larger search's workspace, as it was left
    assert c[4].ws is sess.ws
    for other in (b, c):
        for key in a[0]:
            np.testing.assert_array_equal(np.asarray(a[0][key]), np.asarray(other[0][key]), err_msg=key)
        for (v0, i0), (v1, i1) in zip(a[1], other[1]):
            np.testing.assert_array_equal(v0, v1)
            np.testing.assert_array_equal(i0, i1)
        np.testing.assert_array_equal(_bits(a[2]), _bits(other[2]))
