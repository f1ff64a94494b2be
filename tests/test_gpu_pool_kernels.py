"""The pooling and speaker-vote kernels of csrc/pool.hip against the model of tests/_pool_ref.py, through the C ABI.  pytest -m gpu.

The cases come from the table P.CASES (tests/test_pool_ref_cpu.py shows, without a GPU, that every rule of the model is told
apart from its plausible wrong variants by at least one of them, and that the random-valued ones keep their winners clear of
the summation error).  Comparison (P.compare):
  * exact-valued cases (attention in multiples of 2^-12: every fp32 / float64 sum is exact in any order): ids, weights and
    counts equal to the model's; empty windows, groups and ranges give -1 with the weight the header states;
  * random-valued votes: ids equal; weights within 2 gamma_n sum(w), gamma_n = n u / (1 - n u), u = 2^-24 for the per-token
    vote's fp32 chain and 2^-53 for the grouped vote's float64 sums (kernel and model each err by at most gamma_n sum(w));
    the grouped vote in half mode adds fp16 values, so its weights are bit-equal;
  * pooling, fp32 mode: |got - exact| <= gamma_len sum |a f| (one fmaf chain of len terms); half mode: an fp16 value inside
    [fp16(exact - b), fp16(exact + b)] with the same bound b over the fp16-rounded operands.
Every output has guard rows behind it.

  edge named in the header / issue           case(s)
  tie rules, per-thread loop / wave / merge  vote_ties, groups_ties, major_ties (same thread, lanes of a wave, waves; both id orders)
  winning position beyond 256, S = 600       vote_ties rows 8-11
  all-zero attention, empty window / group   vote_ties rows 13 and 15, groups_ties groups 7-9, major_ties (last range)
  window forms (negative start / both ends   *_windows_T1000_*, *_windows_T300_* (T < S), *_windows_T1_*: the starts of
  negative / start >= T / reversed / T < S)  P.window_starts; major_windows_*: the ranges of P.major_ranges
  half_mode of the grouped vote              groups_half_rounding (fp32 and fp16 winners differ, or tie), every groups case in mode 1
  ids outside [0, num_ids)                   groups_ties groups 10-11, major_ties, groups_num_ids_*, major_num_ids_*
  E > 256, S > 512, num_ids > 256            pool_windows_*_E300, *_S600, *_num_ids_300 and up
  large-LDS launches                         *_num_ids_6008, *_num_ids_13631; the 64 KB boundary: *_num_ids_5455 / 5456 / 5460 / 5461,
                                             vote_largest_S_8192
"""
import numpy as np
import pytest
import torch

from tests import _pool_ref as P
from tests.conftest import golden, has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

GUARD = 3                 # rows behind every output
TAL_OK, TAL_EINVAL = 0, -1
RUNS = [(c["name"], m) for c in P.CASES for m in P.modes(c)]


def dev():
    return torch.device("cuda:0")


def _d(a):
    return torch.from_numpy(np.array(a)).to(dev())      # (a copy: the table's arrays are read-only)


def _guarded(rows, cols, dtype, fill):
    shape = (rows + GUARD,) if cols is None else (rows + GUARD, cols)
    return torch.full(shape, fill, dtype=dtype, device=dev())


def _take(buf, rows, fill, what):
    torch.cuda.synchronize()
    assert bool((buf[rows:] == fill).all()), "%s: the rows behind the output were written" % what
    return buf[:rows].cpu().numpy()


def run_case(lib, N, c, kind, mode):
    """One call of the case's kernel with guarded outputs -> the dict P.compare takes."""
    st = N.stream_handle()
    if kind == "pool":
        out = _guarded(c["N"], c["E"], torch.float32, 777.0)
        attn, cs, feat = _d(c["attn"]), _d(c["cs"]), _d(c["feat"])
        N.check(lib.tal_attn_pool_fwd(N.ptr(attn), N.ptr(cs), N.ptr(feat), c["T"], c["E"], c["N"], c["S"], mode, N.ptr(out), st),
                "tal_attn_pool_fwd")
        return {"out": _take(out, c["N"], 777.0, "out")}
    ids = _d(c["ids"])
    if kind == "vote":
        rows = c["N"]
        oid, ow = _guarded(rows, None, torch.int32, -77), _guarded(rows, None, torch.float32, 777.0)
        attn, cs = _d(c["attn"]), _d(c["cs"])
        N.check(lib.tal_attn_vote_fwd(N.ptr(attn), N.ptr(cs), N.ptr(ids), c["T"], rows, c["S"], N.ptr(oid), N.ptr(ow), st),
                "tal_attn_vote_fwd")
    elif kind == "groups":
        rows = len(c["offsets"]) - 1
        oid, ow = _guarded(rows, None, torch.int32, -77), _guarded(rows, None, torch.float64, 777.0)
        attn, cs, off = _d(c["attn"]), _d(c["cs"]), _d(c["offsets"])
        N.check(lib.tal_attn_vote_groups_fwd(N.ptr(attn), N.ptr(cs), N.ptr(ids), c["T"], c["S"], N.ptr(off), rows, c["num_ids"], mode,
                                             N.ptr(oid), N.ptr(ow), st), "tal_attn_vote_groups_fwd")
    else:
        rows = len(c["ranges"])
        oid, ow = _guarded(rows, None, torch.int32, -77), _guarded(rows, None, torch.float64, 777.0)
        rng = _d(c["ranges"])
        N.check(lib.tal_majority_vote_fwd(N.ptr(ids), c["T"], N.ptr(rng), rows, c["num_ids"], N.ptr(oid), N.ptr(ow), st),
                "tal_majority_vote_fwd")
    return {"id": _take(oid, rows, -77, "out_id"), "weight": _take(ow, rows, 777.0, "out_weight / out_count")}


@pytest.mark.parametrize("name,mode", RUNS, ids=["%s-half%d" % r for r in RUNS])
def test_kernel_against_the_model(name, mode):
    from tal_asrd_amd import _native as N
    case = P.CASE_BY_NAME[name]
    got = run_case(N.lib(), N, P.inputs(name), case["kind"], mode)
    P.compare(case, mode, got)


def test_weights_may_be_null():
    """out_weight / out_count are optional: the ids are the same without them."""
    from tal_asrd_amd import _native as N
    lib, st = N.lib(), N.stream_handle()
    for name in ("vote_ties", "groups_ties", "major_ties"):
        case, c = P.CASE_BY_NAME[name], P.inputs(name)
        want = [v.id for v in P.model(case, 0)]
        ids = _d(c["ids"])
        oid = _guarded(len(want), None, torch.int32, -77)
        if case["kind"] == "vote":
            attn, cs = _d(c["attn"]), _d(c["cs"])
            rc = lib.tal_attn_vote_fwd(N.ptr(attn), N.ptr(cs), N.ptr(ids), c["T"], c["N"], c["S"], N.ptr(oid), None, st)
        elif case["kind"] == "groups":
            attn, cs, off = _d(c["attn"]), _d(c["cs"]), _d(c["offsets"])
            rc = lib.tal_attn_vote_groups_fwd(N.ptr(attn), N.ptr(cs), N.ptr(ids), c["T"], c["S"], N.ptr(off), len(want), c["num_ids"], 0,
                                              N.ptr(oid), None, st)
        else:
            rng = _d(c["ranges"])
            rc = lib.tal_majority_vote_fwd(N.ptr(ids), c["T"], N.ptr(rng), len(want), c["num_ids"], N.ptr(oid), None, st)
        N.check(rc, name)
        assert _take(oid, len(want), -77, name).tolist() == want, name


def test_no_tokens_and_no_groups_write_nothing():
    """N == 0 / G == 0: TAL_OK, outputs untouched."""
    from tal_asrd_amd import _native as N
    lib, st = N.lib(), N.stream_handle()
    c = P.inputs("groups_windows_T1000_S357")
    attn, cs, ids, off = _d(c["attn"]), _d(c["cs"]), _d(c["ids"]), _d(c["offsets"])
    feat = torch.zeros(c["T"], 8, device=dev())
    out = _guarded(0, 8, torch.float32, 777.0)
    oid, ow32, ow64 = _guarded(0, None, torch.int32, -77), _guarded(0, None, torch.float32, 777.0), _guarded(0, None, torch.float64, 777.0)
    assert lib.tal_attn_pool_fwd(N.ptr(attn), N.ptr(cs), N.ptr(feat), c["T"], 8, 0, c["S"], 1, N.ptr(out), st) == TAL_OK
    assert lib.tal_attn_vote_fwd(N.ptr(attn), N.ptr(cs), N.ptr(ids), c["T"], 0, c["S"], N.ptr(oid), N.ptr(ow32), st) == TAL_OK
    assert lib.tal_attn_vote_groups_fwd(N.ptr(attn), N.ptr(cs), N.ptr(ids), c["T"], c["S"], N.ptr(off), 0, 9, 1, N.ptr(oid), N.ptr(ow64),
                                        st) == TAL_OK
    assert lib.tal_majority_vote_fwd(N.ptr(ids), c["T"], N.ptr(off), 0, 9, N.ptr(oid), N.ptr(ow64), st) == TAL_OK
    _take(out, 0, 777.0, "pool"), _take(oid, 0, -77, "out_id"), _take(ow32, 0, 777.0, "out_weight"), _take(ow64, 0, 777.0, "out_count")


def test_sizes_past_the_lds_limits_are_refused_with_a_message():
    """13631 speaker ids are the most the table has room for (12 bytes each + 8 in 160 KB less 256), 8192 the longest window of
    the per-token vote: one more is TAL_EINVAL with a message naming the limit, and nothing is launched."""
    from tal_asrd_amd import _native as N
    lib, st = N.lib(), N.stream_handle()
    c = P.inputs("groups_num_ids_13631")
    attn, cs, ids, off = _d(c["attn"]), _d(c["cs"]), _d(c["ids"]), _d(c["offsets"])
    G = len(c["offsets"]) - 1
    oid, ow = _guarded(G, None, torch.int32, -77), _guarded(G, None, torch.float64, 777.0)
    rc = lib.tal_attn_vote_groups_fwd(N.ptr(attn), N.ptr(cs), N.ptr(ids), c["T"], c["S"], N.ptr(off), G, 13632, 1, N.ptr(oid), N.ptr(ow), st)
    assert rc == TAL_EINVAL and b"13632" in lib.tal_last_error() and b"LDS" in lib.tal_last_error()
    rc = lib.tal_majority_vote_fwd(N.ptr(ids), c["T"], N.ptr(off), 2, 13632, N.ptr(oid), N.ptr(ow), st)
    assert rc == TAL_EINVAL and b"13632" in lib.tal_last_error() and b"LDS" in lib.tal_last_error()
    ow32 = _guarded(G, None, torch.float32, 777.0)
    rc = lib.tal_attn_vote_fwd(N.ptr(attn), N.ptr(cs), N.ptr(ids), c["T"], 1, 8193, N.ptr(oid), N.ptr(ow32), st)
    assert rc == TAL_EINVAL and b"8193" in lib.tal_last_error() and b"8192" in lib.tal_last_error()
    _take(oid, 0, -77, "out_id"), _take(ow, 0, 777.0, "out_weight"), _take(ow32, 0, 777.0, "out_weight")


def test_grouped_vote_refuses_offsets_past_the_attention_rows():
    from tal_asrd_amd import _native as N
    from tal_asrd_amd.wder_format import vote_speaker_ids_grouped
    c = P.inputs("groups_windows_T1000_S357")
    attn, ids, cs = _d(c["attn"]), _d(c["ids"]), _d(c["cs"])
    with pytest.raises(N.NativeError, match="run past the 22 attention rows"):
        vote_speaker_ids_grouped(attn, cs, ids, np.asarray([0, 4, c["N"] + 1]), 9)
    with pytest.raises(N.NativeError, match="run past"):
        vote_speaker_ids_grouped(attn, cs, ids, np.asarray([], dtype=np.int64), 9)
    gid, gw = vote_speaker_ids_grouped(attn, cs, ids, _d(c["offsets"]), 9, half_mode=True)
    P.compare(P.CASE_BY_NAME["groups_windows_T1000_S357"], 1, {"id": gid.cpu().numpy(), "weight": gw.cpu().numpy()})


def test_num_ids_none_equals_the_explicit_count():
    """hyp_dict_to_wder(num_ids=None) sizes the table from the episode's ids: the same words and speakers as num_ids=9, and as a
    table much larger than the ids need."""
    from tal_asrd_amd.tokenizer import SynthTokenizer
    from tal_asrd_amd.wder_format import hyp_dict_to_wder
    g = golden("pool_unit")
    tok = SynthTokenizer()
    toks = g["long_tokens"].tolist()
    hyp = {"utterance": tok.decode(toks), "speakerId": None, "attention": torch.from_numpy(g["long_attn"]),
           "chunkStart": torch.from_numpy(g["long_cs"]), "utteranceTokens": toks}
    feat, ids = _d(g["long_feat"]), _d(g["long_ids"])
    assert int(g["long_ids"].max()) + 1 == 9
    res = [hyp_dict_to_wder(hyp, {}, tok, feat, ids, word_level=True, num_ids=n) for n in (None, 9, 6008)]
    for r in res:
        assert [(w[0], w[1][1], w[2]) for w in r] == [(w[0], w[1][1], w[2]) for w in res[1]]
        assert all(torch.equal(a[1][0], b[1][0]) for a, b in zip(r, res[1]))
    assert [w[1][1] for w in res[0]] == g["long_word_spk"].tolist()
