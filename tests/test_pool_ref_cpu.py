"""tests/_pool_ref.py against the reference's own outputs, and the case table of tests/test_gpu_pool_kernels.py against the
model's knobs.  Runs without a GPU.

  * the model on the inputs recorded in tests/golden/pool_unit.* and aligned_unit.* (written by the reference's
    get_hyp_dict_wder and by its aligned branch): voted word speakers and majority votes identical, embeddings within one
    fp16 ulp (the reference pools in half precision with its own summation order);
  * every knob of the model (a rule switched to a plausible wrong variant) changes what at least one case of the table
    expects, by more than the comparison of the GPU test lets pass -- an input that cannot tell the right rule from the
    wrong one is no test of that rule;
  * the random-valued cases keep the winner clear of the runner-up by more than twice the summation bound, in every row
    and group, so that the ids of all of them are compared."""
import json
import os
from collections import defaultdict

import numpy as np
import pytest

from tests import _pool_ref as P
from tests.conftest import GOLDEN, golden

HALF_ULP = 2.0 ** -10     # relative spacing of fp16


def _half_close(model_exact, want, what):
    got = P.f16(model_exact)
    np.testing.assert_allclose(got, want, rtol=HALF_ULP, atol=2.0 ** -24, err_msg=what)
    return float(np.mean(got == want))


@pytest.mark.parametrize("name", ["long", "short_wrap", "short_zero"])
def test_model_matches_the_recorded_unaligned_outputs(name):
    from tal_asrd_amd.tokenizer import SynthTokenizer
    from tal_asrd_amd.wder_format import split_words
    g = golden("pool_unit")
    attn, cs, feat, ids = (g[name + k] for k in ("_attn", "_cs", "_feat", "_ids"))
    exact, _, _ = P.pool(attn, cs, feat, half=True)
    equal = _half_close(exact, g[name + "_utt_emb"], "utterance embeddings")
    assert equal > 0.99                      # (the reference's half matmul sums in another order: a few differ by an ulp)
    words = split_words(g[name + "_tokens"].tolist(), SynthTokenizer())
    assert [b - a for a, b, _ in words] == g[name + "_word_ntok"].tolist()
    if not words:
        assert g[name + "_word_spk"].size == 0
        return
    offsets = [w[0] for w in words] + [words[-1][1]]
    votes = P.vote_groups(attn, cs, ids, offsets, 9, half=True)
    assert [v.id for v in votes] == g[name + "_word_spk"].tolist()
    _half_close(np.concatenate([exact[a:b] for a, b, _ in words]), g[name + "_word_emb"], "word embeddings")


def test_model_matches_the_recorded_majority_votes():
    g = golden("pool_unit")
    votes = P.majority(g["major_ids"], g["major_ranges"], 5)
    assert [v.id for v in votes] == g["major_votes"].tolist()
    ids = g["major_ids"].tolist()
    for (a, b), v in zip(g["major_ranges"].tolist(), votes):
        assert v.weight == (ids[a:b].count(v.id) if v.id >= 0 else 0)


def test_model_matches_the_recorded_aligned_branch():
    """Speaker ids (given, or the majority vote over ids[st_frame:e_frame]) and embeddings (attention pooling or the plain
    feature slice, in half precision) of the reference script's own pickle, in its order (per episode, by utterance_start)."""
    g = golden("aligned_unit")
    with open(os.path.join(GOLDEN, "aligned_unit.json")) as f:
        meta = json.load(f)
    per_episode = defaultdict(list)
    episodes = []
    n_votes = 0
    for k, ex in enumerate(meta["examples"]):
        ep = ex["episode"]
        if ep not in episodes:
            episodes.append(ep)
        valid = [h for h in ex["hyps"] if h["utterance"].strip()]
        if not valid:
            continue
        h, = valid
        st = int(ex["utterance_start"] / 0.08)
        en = max(int(max(0.0, ex["utterance_end"] - 1.0) / 0.08), st + 1)
        spk = h["speakerId"]
        if spk is None:
            spk = P.majority(g["ids_" + ep], [[st, en]], 6)[0].id
            n_votes += 1
        if h["has_attention"]:
            emb = P.f16(P.pool(g["attn_%d" % k], g["cs_%d" % k], g["feat_" + ep], half=True)[0])
        else:
            emb = P.f16(g["feat_" + ep][st:en])
        per_episode[ep].append((ex["utterance_start"], spk, emb))
    assert n_votes >= 3
    assert len(episodes) == len(meta["wder_input"])
    for gi, (ep, want) in enumerate(zip(episodes, meta["wder_input"])):
        hyps = sorted(per_episode[ep], key=lambda x: x[0])
        assert len(hyps) == len(want["hyps"])
        for hi, ((_, spk, emb), w) in enumerate(zip(hyps, want["hyps"])):
            assert int(spk) == w["speaker"], (gi, hi)
            ref = g["out_emb_%d_%d" % (gi, hi)]
            assert emb.shape == ref.shape, (gi, hi)
            np.testing.assert_allclose(emb, ref, rtol=HALF_ULP, atol=2.0 ** -24)


def _runs():
    return [(c, m) for c in P.CASES for m in P.modes(c)]


def _rejected(case, mode, rules):
    try:
        P.compare(case, mode, P.outputs(case, mode, rules))
    except AssertionError:
        return True
    return False


def test_the_comparison_accepts_the_model_itself():
    for case, mode in _runs():
        P.compare(case, mode, P.outputs(case, mode))


@pytest.mark.parametrize("knob", sorted(P.KNOBS))
def test_every_knob_is_discriminated_by_a_table_case(knob):
    hits = [(c["name"], m) for c, m in _runs() if knob in P.KNOBS_OF[c["kind"]] and _rejected(c, m, P.KNOBS[knob])]
    kinds = {P.CASE_BY_NAME[n]["kind"] for n, _ in hits}
    want = {k for k, v in P.KNOBS_OF.items() if knob in v}
    assert kinds == want, "%s is told apart for %s only, not for %s" % (knob, sorted(kinds), sorted(want - kinds))
    for c, m in _runs():                 # the cases built for this rule must each tell it apart, in every mode they run in
        if knob in c["must"] and not (knob == "no_fp16" and m == 0):
            assert (c["name"], m) in hits, (c["name"], m)


def test_planted_ties_are_ties_and_each_placement_tells_the_rules_apart():
    """Row by row: the planted rows have a zero margin, and the right rule's winner differs from both wrong rules' winners
    in at least one of the two id orders of each placement."""
    for name, knobs, n_planted in (("vote_ties", ("vote_tie_last", "vote_tie_lowest"), 12),
                                   ("groups_ties", ("groups_tie_first", "groups_tie_lowest"), 6),
                                   ("major_ties", ("major_tie_last", "major_tie_lowest"), 8)):
        case = P.CASE_BY_NAME[name]
        right = P.model(case, 0)
        assert all(v.margin == 0 for v in right[:n_planted]), name
        for knob in knobs:
            wrong = P.model(case, 0, P.KNOBS[knob])
            for k in range(0, n_planted, 2):             # (x, y) and (y, x) of one placement
                assert right[k].id != wrong[k].id or right[k + 1].id != wrong[k + 1].id, (name, knob, k)
            if "lowest" not in knob:
                assert all(right[k].id != wrong[k].id for k in range(n_planted)), (name, knob)


def test_half_rounding_case_flips_the_winner():
    case = P.CASE_BY_NAME["groups_half_rounding"]
    assert [v.id for v in P.model(case, 0)] == [8, 4]
    assert [v.id for v in P.model(case, 1)] == [3, 6]
    assert P.model(case, 1)[1].margin == 0 and P.model(case, 1)[0].margin > 0


def test_random_cases_keep_the_winner_clear_of_the_runner_up():
    n = 0
    for case, mode in _runs():
        if case["kind"] not in ("vote", "groups") or case["exact"]:
            continue
        u = P.vote_unit(case)
        for k, v in enumerate(P.model(case, mode)):
            if v.id < 0:
                continue
            assert v.margin > 2 * P.gamma(v.n, u) * v.total, (case["name"], mode, k, v)
            n += 1
    assert n >= 20


def test_the_table_reaches_the_shapes_where_the_kernels_change_path():
    seen = defaultdict(set)
    for case in P.CASES:
        c = P.inputs(case["name"])
        for key in ("S", "T", "E", "N", "num_ids"):
            if key in c:
                seen[case["kind"], key].add(c[key])
    for kind in ("vote", "groups", "pool"):
        assert {1, 64, 257, 357, 600} <= seen[kind, "S"], kind
        assert {1, 300, 1000} <= seen[kind, "T"], kind
    assert {1, 127, 128, 129, 300} <= seen["pool", "E"]
    assert 1 in seen["pool", "N"] and 8192 in seen["vote", "S"]
    for kind in ("groups", "major"):
        assert {1, 9, 300, 6008, 13631, 5455, 5456, 5460, 5461} <= seen[kind, "num_ids"], kind
    # window forms: every start of window_starts() gives the slice python gives
    for T, S in ((1000, 357), (300, 357), (1, 64), (300, 600)):
        x = list(range(T))
        for cs in P.window_starts(T, S).tolist():
            a, n = P.window(cs, S, T)
            assert x[cs:cs + S] == x[a:a + n], (T, S, cs)
    a, n = P.window(-358, 357, 300)
    assert n == 299          # start and end both negative, T <= S: not empty
