"""CPU checks around the device-resident beam search (System.generate(search="device"), tal_beam_ctx): the numpy model of the
loop's bookkeeping (tests/_beam_ref.py) behaves as tal/asr/system.py:141-219 does, and the boundary of the new entry points --
keyword validation before the GPU is touched, struct layout, argument limits -- holds without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests._beam_ref import BeamRef, topk_ref
from tests.conftest import ROOT


def _logprobs(rng, rows, V):
    x = rng.standard_normal((rows, V)).astype(np.float32)
    return (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)


def _run(ref, rng, steps, boost=None, spk=False):
    """Drive the model with its own selections; the terminate token is out of reach (-60) except in the rows boost(step) names (+60)."""
    for t in range(steps):
        rows = ref.B * ref.cur_beam
        lp = _logprobs(rng, rows, ref.V)
        if ref.terminate is not None:
            lp[:, ref.terminate] -= 60.0
        if boost is not None:
            for r in boost(t):
                if r < rows:
                    lp[r, ref.terminate] += 120.0
        vals, idx = topk_ref(lp, ref.scores[:rows] if ref.step else np.zeros(rows, np.float32), ref.mask(), ref.B, ref.cur_beam, ref.beam)
        ref.advance(vals, idx, rng.standard_normal((rows, ref.ns)).astype(np.float32) if spk else None)


def test_beam1_is_the_argmax_chain():
    rng = np.random.default_rng(0)
    B, V, steps = 3, 50, 7
    ref = BeamRef(np.zeros((B, 1), np.int64), 1, V)
    want = [np.zeros(B, np.int64)]
    total = np.zeros(B, np.float32)
    for _ in range(steps):
        lp = _logprobs(rng, B, V)
        vals, idx = topk_ref(lp, ref.scores, ref.mask(), B, 1, 1)
        arg = lp.argmax(-1)
        np.testing.assert_array_equal(idx[:, 0], arg)
        total = (lp[np.arange(B), arg] + total).astype(np.float32)
        np.testing.assert_array_equal(vals[:, 0], total)
        ref.advance(vals, idx)
        want.append(arg)
    np.testing.assert_array_equal(ref.tokens, np.stack(want, 1))
    assert ref.step == steps and not ref.stopped and not ref.records


def test_topk_order_ties_mask_and_nan():
    lp = np.array([[0.0, 1.0, 1.0, -np.inf], [1.0, np.nan, 0.5, 1.0]], np.float32)
    vals, idx = topk_ref(lp, np.zeros(2, np.float32), None, 1, 2, 8)
    # ties: lowest flat index first; -inf is a candidate like any other; the NaN comes last and is reported as -inf
    np.testing.assert_array_equal(idx[0], [1, 2, 4, 7, 6, 0, 3, 5])
    np.testing.assert_array_equal(vals[0], np.array([1, 1, 1, 1, 0.5, 0, -np.inf, -np.inf], np.float32))
    vals, idx = topk_ref(lp, np.zeros(2, np.float32), np.array([True, True]), 1, 2, 3)       # all masked: lowest indices, -inf
    np.testing.assert_array_equal(idx[0], [0, 1, 2])
    assert np.isneginf(vals).all()


def test_a_slot_finishes_once_and_the_loop_stops_with_the_last_slot():
    rng = np.random.default_rng(1)
    B, beam, V, term = 2, 3, 40, 1
    ref = BeamRef(np.zeros((B, 1), np.int64), beam, V, terminate_token=term)
    # item 0 finishes as a whole at step 2, item 1 at step 4; the terminate token is boosted again later on
    _run(ref, rng, 9, boost=lambda t: {2: [0, 1, 2], 4: [3, 4, 5], 5: range(6), 6: range(6)}.get(t, []))
    assert ref.stopped and ref.step == 5                         # the step at which the last slot finished; later calls changed nothing
    assert ref.tokens.shape == (B * beam, 1 + 5)
    slots = [r["slot"] for r in ref.records]
    assert sorted(slots) == list(range(B * beam)) and len(set(slots)) == len(slots)       # one record per slot
    assert [r["step"] for r in ref.records] == sorted(r["step"] for r in ref.records)
    for r in ref.records:
        assert r["row"][-1] == term and len(r["row"]) == 1 + r["step"] + 1
        assert r["step"] == (2 if r["slot"] < beam else 4)


def test_a_done_slot_adds_no_second_record():
    B, beam, V, term = 1, 2, 10, 1
    ref = BeamRef(np.zeros((B, 1), np.int64), beam, V, terminate_token=term)
    f32 = np.float32
    ref.advance(np.array([[-1, -2]], f32), np.array([[term, 5]]))             # slot 0 finishes at step 0
    assert ref.done.tolist() == [True, False] and len(ref.records) == 1
    # slot 0 (done) receives the terminate token again, from the live row: no record, the flag stays with the slot
    ref.advance(np.array([[-3, -4]], f32), np.array([[1 * V + term, 1 * V + 7]]))
    assert len(ref.records) == 1 and ref.done.tolist() == [True, False] and not ref.stopped
    np.testing.assert_array_equal(ref.tokens, [[0, 5, term], [0, 5, 7]])
    ref.advance(np.array([[-5, -6]], f32), np.array([[0 * V + 3, 1 * V + term]]))     # slot 1 finishes: stop
    assert ref.stopped and ref.step == 3 and [r["slot"] for r in ref.records] == [0, 1]
    assert ref.records[1]["score"] == f32(-6) and ref.records[1]["row"].tolist() == [0, 5, 7, term]
    before = (ref.tokens.copy(), ref.scores.copy())
    ref.advance(np.array([[0, 0]], f32), np.array([[2, 3]]))
    np.testing.assert_array_equal(ref.tokens, before[0])
    np.testing.assert_array_equal(ref.scores, before[1])
    assert ref.step == 3


@pytest.mark.parametrize("B,beam,ns", [(1, 1, 5), (2, 3, 7), (3, 4, 2)])
def test_parent_chain_gather_equals_index_select_and_cat(B, beam, ns):
    rng = np.random.default_rng(2 + beam)
    ref = BeamRef(np.zeros((B, 1), np.int64), beam, 30, terminate_token=1, num_speakers=ns)
    _run(ref, rng, 8, boost=lambda t: [t % (B * beam)] if t in (3, 5) and B * beam > 1 else [], spk=True)
    assert ref.step == 8
    for step in (0, 3, 7):
        cat_form = ref.spk_embeds[:, :step + 1] if step == 7 else None
        for slot in range(ref.R):
            got = ref.gather(slot, step)
            assert got.shape == (step + 1, ns)
            if cat_form is not None:
                np.testing.assert_array_equal(got, cat_form[slot])
    # the torch form the host loop uses (index_select + cat), replayed from the stored rows and parents
    hist = None
    for s in range(ref.step):
        rows = torch.from_numpy(ref.spk_rows[s]).unsqueeze(1)
        hist = rows if hist is None else torch.cat((hist.index_select(0, torch.from_numpy(ref.parents[s])), rows), dim=1)
    np.testing.assert_array_equal(hist.numpy(), np.stack([ref.gather(slot, ref.step - 1) for slot in range(ref.R)]))
    for r in ref.records:
        np.testing.assert_array_equal(ref.gather(r["slot"], r["step"]), r["spk"])


def test_generate_rejects_an_unknown_search_mode_without_a_gpu():
    from tal_asrd_amd.system import System
    from tal_asrd_amd import transcribe
    import inspect
    with pytest.raises(ValueError, match="search"):
        System(model=None).generate(None, None, None, length=4, search="bogus")
    for fn in (transcribe.transcribe_batch, transcribe.transcribe_file, System.generate):
        assert inspect.signature(fn).parameters["search"].default == "host"


def test_beam_ctx_layout_matches_header(tmp_path):
    """The ctypes mirror of tal_beam_ctx against the header as gcc lays it out: sizeof and the offset of every field."""
    from tal_asrd_amd import _native
    mirror = _native.BeamCtx
    assert C.sizeof(mirror) == 6 * 4 + 4 * 8 + 6 * 8 + 2 * 8 + 6 * 8 + 8 + 4 + 4      # ints, workspace + size + 2 host words, state, tokens[2], selection + partials + speaker, state_bytes, seq + pad
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tal_asrd.h"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(tal_beam_ctx));']
    for fname, _ in mirror._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(tal_beam_ctx, %s));' % (fname, fname))
    lines += ['return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict((ln.split()[0], int(ln.split()[1])) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert got["sizeof"] == C.sizeof(mirror)
    for fname, _ in mirror._fields_:
        assert got[fname] == getattr(mirror, fname).offset, fname


def _ctx(B, beam, L0, length, V, ns=0):
    from tal_asrd_amd import _native as N
    c = N.BeamCtx()
    c.B, c.beam, c.L0, c.length, c.V, c.num_speakers = B, beam, L0, length, V, ns
    return c


def test_limit_violations_return_einval():
    """Argument checks come before any device work, so they are testable here: R <= 512, beam <= 64, beam <= cur_beam * V, and
    the plain shape / pointer errors."""
    from tal_asrd_amd import _native as N
    lib = N.lib()
    assert lib.tal_beam_workspace_bytes(2, 3, 1, 12, 255, 0) > 0
    assert lib.tal_beam_workspace_bytes(2, 3, 1, 12, 255, 7) > lib.tal_beam_workspace_bytes(2, 3, 1, 12, 255, 0)
    assert lib.tal_beam_workspace_bytes(64, 8, 1, 12, 300, 0) > 0                 # R = 512
    for bad in ((65, 8, 1, 12, 300, 0), (1, 65, 1, 12, 300, 0), (0, 1, 1, 12, 300, 0), (1, 1, 0, 12, 300, 0), (1, 1, 1, 0, 300, 0),
                (1, 1, 1, 12, 0, 0), (1, 1, 1, 12, 300, -1)):
        assert lib.tal_beam_workspace_bytes(*bad) == 0, bad
    fake = C.c_void_p(4096)      # never dereferenced: every call below is refused first
    for shape, what in (((65, 8, 1, 12, 300), b"512"), ((1, 65, 1, 12, 300), b"64"), ((1, 1, 1, 0, 300), b"bad shape")):
        c = _ctx(*shape)
        assert lib.tal_beam_init_fwd(C.byref(c), fake, None) == -1
        assert what in lib.tal_last_error(), lib.tal_last_error()
        assert lib.tal_beam_select_fwd(C.byref(c), 0, 1, fake, None, 0, None) == -1
        assert lib.tal_beam_advance_fwd(C.byref(c), 0, 1, -1, None, None) == -1
    c = _ctx(2, 3, 1, 12, 255)
    assert lib.tal_beam_init_fwd(C.byref(c), fake, None) == -1 and b"workspace" in lib.tal_last_error()       # no workspace
    c.workspace, c.workspace_bytes = 4096, lib.tal_beam_workspace_bytes(2, 3, 1, 12, 255, 0) - 1
    assert lib.tal_beam_init_fwd(C.byref(c), fake, None) == -1 and b"workspace" in lib.tal_last_error()       # too small
    c.workspace_bytes += 1
    assert lib.tal_beam_init_fwd(C.byref(c), None, None) == -1 and b"null pointer" in lib.tal_last_error()
    # steps: outside [0, length), a cur_beam that is neither the seed rows of step 0 nor beam, more beams than candidates,
    # a context that never went through init
    assert lib.tal_beam_select_fwd(C.byref(c), 12, 3, fake, None, 0, None) == -1 and b"step" in lib.tal_last_error()
    assert lib.tal_beam_select_fwd(C.byref(c), 1, 1, fake, None, 0, None) == -1 and b"cur_beam" in lib.tal_last_error()
    assert lib.tal_beam_select_fwd(C.byref(c), 0, 2, fake, None, 0, None) == -1 and b"cur_beam" in lib.tal_last_error()
    assert lib.tal_beam_select_fwd(C.byref(c), 0, 1, fake, None, 0, None) == -1 and b"tal_beam_init_fwd" in lib.tal_last_error()
    assert lib.tal_beam_advance_fwd(C.byref(c), 0, 1, -1, None, None) == -1 and b"tal_beam_init_fwd" in lib.tal_last_error()
    few = _ctx(1, 3, 1, 4, 2)
    few.workspace, few.workspace_bytes = 4096, lib.tal_beam_workspace_bytes(1, 3, 1, 4, 2, 0)
    assert lib.tal_beam_select_fwd(C.byref(few), 0, 1, fake, None, 0, None) == -1 and b"candidates" in lib.tal_last_error()
    assert lib.tal_beam_gather_spk_fwd(C.byref(c), fake, 1, fake, None) == -1 and b"speaker" in lib.tal_last_error()
