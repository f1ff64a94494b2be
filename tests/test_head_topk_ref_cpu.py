"""CPU side of the per-row top-k / log-sum-exp of the speaker head (tal_spk_topk_fwd, tal_topk_lse_rows): the float64 model and its
case table (tests/_head_topk_ref.py) tell the semantics apart from their plausible wrong variants, the random cases keep to the cap
on unclear rows, and the boundary is in place -- symbols, binding table, options, argument checks before any launch, no CPU fallback."""
import numpy as np
import pytest
import torch

from tests import _head_topk_ref as R


def test_the_model_passes_its_own_comparison():
    for name in R.CASES:
        _, _, _, ref = R.build(name)
        assert R.compare(ref, ref.ids, ref.logp, ref.lse) == [], name
    for name in R.ROWS_CASES:
        _, ref = R.build_rows(name)
        assert R.compare(ref, ref.ids, ref.logp, ref.lse) == [], name


def test_fp32_rounding_of_the_model_stays_inside_the_bound():
    """The bound is not vacuous the other way round either: the model's results rounded to fp32, and its logits recomputed in fp32 by
    numpy, pass."""
    for name in ("random-300-6008-8", "exact-300-6008-8", "masked-129-6008-8-ragged", "random-1-5-1"):
        feat, W, b, ref = R.build(name)
        assert R.compare(ref, ref.ids, ref.logp.astype(np.float32), ref.lse.astype(np.float32)) == [], name
        z32 = (feat @ W.T + b).astype(np.float32)
        ids, logp, lse = R.topk_lse(z32.astype(np.float64), ref.k)
        assert R.compare(ref, ids, logp, lse) == [], name


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_every_wrong_variant_fails_some_case(variant):
    failed = [name for name in R.CASES if R.compare(R.build(name)[3], *R.build(name)[3].wrong(variant))]
    assert failed, "no case tells the model from the variant '%s'" % variant


def test_the_planted_pairs_give_ln_2():
    for name in ("exact-300-6008-2-two", "exact-33-300-1-two"):
        _, _, _, ref = R.build(name)
        plants = list(R.CASES[name]["plants"])
        assert (ref.ids[:, 0] == plants[0]).all()
        if ref.k > 1:
            assert (ref.ids[:, 1] == plants[1]).all()
        np.testing.assert_allclose(ref.lse, ref.z[:, plants[0]] + np.log(2.0), atol=1e-9, rtol=0)
        np.testing.assert_array_equal(ref.z[:, plants[0]], ref.z[:, plants[1]])


def test_exact_cases_have_ties_at_every_rank():
    _, _, _, ref = R.build("exact-300-6008-16")
    top = -np.sort(-ref.z, axis=1)[:, :17]
    tied = (top[:, :-1] == top[:, 1:]).any(axis=0)
    # some row ties at every boundary, the k-th included -- except behind the 12 planted winners, which stand 24 above the rest
    assert tied[:11].all() and not tied[11] and tied[12:].all()
    assert set(ref.ids[0, :12].tolist()) == set(R._plants(6008))


def test_unclear_rows_stay_under_the_cap():
    shares = {name: R.build(name)[3].unclear_share for name, c in R.CASES.items() if c["kind"] != "exact"}
    shares["repeat"] = R.build_repeat()[3].unclear_share
    for name, s in shares.items():
        assert s <= R.UNCLEAR_CAP, (name, s)
    # the float64 model's shares at the shapes the issue lists (its table, rounded up)
    for name, cap in (("random-300-6008-8", 0.035), ("random-300-6008-4", 0.015), ("random-129-300-8", 0.01), ("random-129-129-8", 0.005),
                      ("random-33-33-8", 0.035), ("repeat", 0.015)):
        assert shares[name] <= cap, (name, shares[name])


def test_the_table_covers_the_shapes_pairwise():
    seen = [(c["M"], c["S"], c["k"]) for c in R.CASES.values()]
    for M in R.MS:
        for S in R.SS:
            assert any(m == M and s == S for m, s, _ in seen)
        for k in R.KS:
            assert any(m == M and kk == k for m, _, kk in seen), (M, k)
    for S in R.SS:
        for k in R.KS:
            if k <= S:
                assert any(s == S and kk == k for _, s, kk in seen), (S, k)
    assert (300, 6008, 8) in seen


# ------------------------------------------------------------------ the boundary
def test_symbols_and_binding_table():
    from tal_asrd_amd import _native as N
    lib = N.lib()
    for name in ("tal_spk_topk_workspace_bytes", "tal_spk_topk_fwd", "tal_topk_lse_rows"):
        assert name in N.SIGNATURES and hasattr(lib, name), name
    assert N.TAL_TOPK_MAX == 16
    assert lib.tal_spk_topk_workspace_bytes(300, 6008, 128, 8) >= 300 * 6008 * 4
    # the generic form's logits never take more than 64 MiB
    assert lib.tal_spk_topk_workspace_bytes(44983, 6008, 96, 8) <= 64 << 20


def test_arguments_are_checked_before_any_launch():
    from tal_asrd_amd import _native as N
    lib = N.lib()
    for k, S in ((0, 10), (17, 6008), (6, 5), (-1, 10)):
        assert lib.tal_spk_topk_fwd(None, 4, 128, None, None, S, k, None, None, None, None, 0, None) == -1, (k, S)
        assert b"k=" in lib.tal_last_error()
        assert lib.tal_topk_lse_rows(None, 4, S, k, None, None, None, None) == -1, (k, S)
        assert b"k=" in lib.tal_last_error()
    assert lib.tal_spk_topk_fwd(None, 0, 128, None, None, 10, 4, None, None, None, None, 0, None) == 0        # M == 0
    assert lib.tal_topk_lse_rows(None, 0, 10, 4, None, None, None, None) == 0
    assert lib.tal_spk_topk_fwd(None, 4, 128, None, None, 10, 4, None, None, None, None, 0, None) == -1
    assert b"null pointer" in lib.tal_last_error()


def test_the_two_options_enumerate():
    from tal_asrd_amd import _native as N
    lib = N.lib()
    names = []
    while lib.tal_option_name(len(names)):
        names.append(lib.tal_option_name(len(names)).decode())
    assert "head_topk_form" in names and "head_topk_grid" in names
    assert N.get_option("head_topk_form") == 0 and N.get_option("head_topk_grid") == 0
    try:
        N.set_option("head_topk_form", 2)
        N.set_option("head_topk_grid", 7)
        assert N.get_option("head_topk_form") == 2 and N.get_option("head_topk_grid") == 7
        assert lib.tal_set_option(b"head_topk_form", 3) == -1 and lib.tal_set_option(b"head_topk_grid", -1) == -1
        assert N.get_option("head_topk_form") == 2 and N.get_option("head_topk_grid") == 7
    finally:
        N.set_option("head_topk_form", 0)
        N.set_option("head_topk_grid", 0)


def test_no_cpu_fallback():
    from tal_asrd_amd import NativeError, SDModel, ops
    with pytest.raises(NativeError):
        SDModel().speaker_topk(torch.zeros(1, 16000))
    with pytest.raises(NativeError):
        ops.spk_topk(torch.zeros(4, 128), torch.zeros(10, 128), torch.zeros(10), 4)
    with pytest.raises(NativeError):
        ops.topk_lse_rows(torch.zeros(4, 10), 4)
