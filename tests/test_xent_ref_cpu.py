"""CPU side of teacher-forced scoring without the logits (tal_xent_rows_fwd, tal_xent_lse_rows, tal_lm_xent_fwd): the float64 model
and its case table (tests/_xent_ref.py) agree with torch's cross-entropy, tell the semantics apart from their plausible wrong
variants, the random cases keep to the cap on unclear rows, and the boundary is in place -- header, symbols, binding table, options,
argument checks before any launch, no CPU fallback."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _xent_ref as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tal_asrd.h")
SYMBOLS = ("tal_xent_rows_workspace_bytes", "tal_xent_rows_fwd", "tal_xent_lse_rows", "tal_lm_xent_workspace_bytes", "tal_lm_xent_fwd")


def test_the_model_agrees_with_torch_in_float64():
    """nll against torch.nn.functional.cross_entropy(reduction='none'), lse against torch.logsumexp, top1 against torch.argmax
    where the maximum is unique, on the rows whose target names a column."""
    for name in R.CASES:
        _, _, _, target, ref = R.build(name)
        z = torch.from_numpy(ref.z)
        np.testing.assert_allclose(ref.lse, torch.logsumexp(z, dim=1).numpy(), rtol=0, atol=1e-11, err_msg=name)
        ok = (target >= 0) & (target < ref.N)
        assert ok.any() or ref.M == 1, name
        ce = torch.nn.functional.cross_entropy(z[ok], torch.from_numpy(target[ok]), reduction="none").numpy()
        fin = np.isfinite(ce)
        np.testing.assert_allclose(ref.nll[ok][fin], ce[fin], rtol=0, atol=1e-11, err_msg=name)
        assert np.array_equal(ref.nll[ok][~fin], ce[~fin]), name           # (+inf on a masked column on both sides)
        assert (ref.nll[target < 0] == 0.0).all() and np.isinf(ref.nll[target >= ref.N]).all(), name
        unique = (ref.z == ref.zmax[:, None]).sum(axis=1) == 1
        assert np.array_equal(ref.top1[unique], torch.argmax(z, dim=1).numpy()[unique]), name
        # ignore_index is the library's "negative target": the two reductions of the validation loss
        t = torch.from_numpy(np.where(ok, target, -100))
        if ok.any() and np.isfinite(ref.nll).all():
            mean = torch.nn.functional.cross_entropy(z, t, ignore_index=-100, reduction="sum").item()
            np.testing.assert_allclose(ref.nll[ok].sum(), mean, rtol=1e-12, atol=1e-9, err_msg=name)


def test_the_model_passes_its_own_comparison():
    for name in R.CASES:
        ref = R.build(name)[4]
        assert R.compare(ref, ref.nll, ref.lse, ref.top1) == [], name
    for name in R.ROWS_CASES:
        ref = R.build_rows(name)[2]
        assert R.compare(ref, ref.nll, ref.lse, ref.top1) == [], name


def test_fp32_rounding_of_the_model_stays_inside_the_bound():
    """The bound is not vacuous the other way round either: the model's results rounded to fp32, and its logits recomputed in fp32 by
    numpy, pass."""
    for name in ("random-257-1000-128-rb", "exact-257-1000-64-rb", "spread-131-1000-64", "masked-131-300-128", "random-1-1-64"):
        feat, W, b, target, ref = R.build(name)
        assert R.compare(ref, ref.nll.astype(np.float32), ref.lse.astype(np.float32), ref.top1) == [], name
        z32 = (feat[:, :W.shape[1]] @ W.T + b).astype(np.float32)
        assert R.compare(ref, *R.xent(z32.astype(np.float64), target)) == [], name


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_every_wrong_variant_fails_some_case(variant):
    failed = [name for name in R.CASES if R.compare(R.build(name)[4], *R.build(name)[4].wrong(variant))]
    assert failed, "no case tells the model from the variant '%s'" % variant


def test_unclear_rows_stay_under_the_cap():
    for name, c in R.CASES.items():
        if c["kind"] not in ("exact", "planted"):
            assert R.build(name)[4].unclear_share <= R.UNCLEAR_CAP, (name, R.build(name)[4].unclear_share)
    for name in R.ROWS_CASES:
        if name.startswith("random"):
            assert R.build_rows(name)[2].unclear_share <= R.UNCLEAR_CAP, name


def test_the_table_covers_what_it_claims():
    seen = [(c["E"], c["N"], c["M"]) for c in R.CASES.values()]
    for E in R.FUSED_E + R.GENERIC_E:
        for N in R.NS:
            assert any(e == E and n == N for e, n, _ in seen), (E, N)
        for M in R.MS:
            assert any(e == E and m == M for e, _, m in seen), (E, M)
    assert any(c.get("ldf", c["E"]) > c["E"] and c["E"] in R.FUSED_E for c in R.CASES.values())
    assert any(c.get("ldf", c["E"]) > c["E"] and c["E"] in R.GENERIC_E for c in R.CASES.values())
    # targets: column 0, N - 1, 127, 128, the ragged tail, skipped and past the head, in one case at least each
    _, _, _, t, ref = R.build("random-257-300-64")
    for want in (0, 299, 127, 128):
        assert (t == want).any(), want
    assert ((t > 256) & (t < 299)).any() and (t < 0).any() and (t >= 300).any() and (t > 2 ** 31).any() and (t < -2 ** 31).any()
    # the spread cases do spread, and an unrescaled sum is wrong there by far more than the bound
    ref = R.build("spread-131-1000-64")[4]
    assert ref.z.max() > 70 and ref.z.min() < -70
    # planted: the maximum and the target sit in the first and the last tile, alternating
    for name in (n for n, c in R.CASES.items() if c["kind"] == "planted"):
        _, _, _, t, ref = R.build(name)
        assert (ref.top1[0::2] == 5).all() and (t[0::2] == ref.N - 3).all() and (ref.top1[1::2] == ref.N - 3).all() and (t[1::2] == 5).all()
        assert 5 // 128 == 0 and (ref.N - 3) // 128 == (ref.N - 1) // 128
    # masked: some targets sit on -inf columns (nll = +inf) and every row keeps a finite column
    for name in (n for n, c in R.CASES.items() if c["kind"] == "masked"):
        _, _, b, t, ref = R.build(name)
        on = (t >= 0) & (t < ref.N)
        assert np.isinf(b[t[on]]).any() and np.isfinite(ref.lse).all(), name
    # exact: equal winners, the lowest index is the model's
    ref = R.build("exact-257-1000-64-rb")[4]
    assert (ref.top1 == 3).all() and ((ref.z == ref.zmax[:, None]).sum(axis=1) == len(R._plants(1000))).all()


# ------------------------------------------------------------------ the boundary
def test_the_header_declares_the_entry_points_and_options():
    text = open(HEADER).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, text), name
    options = text[text.index("Process-wide behaviour switches"):text.index("int tal_set_option")]
    assert "xent_form" in options and "xent_grid" in options
    assert options.index("head_topk_form") < options.index("xent_form")


def test_symbols_and_binding_table():
    from tal_asrd_amd import _native as N
    lib = N.lib()
    for name in SYMBOLS:
        assert name in N.SIGNATURES and hasattr(lib, name), name
    assert lib.tal_xent_rows_workspace_bytes(300, 1000, 32) >= 300 * 1000 * 4
    # the generic form's logits never take more than 64 MiB; the fused partials of the joint vocabulary are far smaller than the logits
    assert lib.tal_xent_rows_workspace_bytes(8192, 16008, 256) <= 64 << 20
    assert lib.tal_lm_xent_workspace_bytes(8192, 512, 64, 16008) <= (64 << 20) + 8192 * 64 * 4
    assert lib.tal_xent_rows_workspace_bytes(0, 10, 64) == 0


def test_arguments_are_checked_before_any_launch():
    from tal_asrd_amd import _native as N
    lib = N.lib()
    for M, ldf, E, n in ((-1, 64, 64, 10), (4, 64, 0, 10), (4, 64, 64, 0), (4, 63, 64, 10)):
        assert lib.tal_xent_rows_fwd(None, M, ldf, E, None, None, n, None, None, None, None, None, 0, None) == -1, (M, ldf, E, n)
        assert b"bad shape" in lib.tal_last_error()
    assert lib.tal_xent_rows_fwd(None, 0, 64, 64, None, None, 10, None, None, None, None, None, 0, None) == 0        # M == 0
    assert lib.tal_xent_lse_rows(None, 0, 10, None, None, None, None, None) == 0
    assert lib.tal_lm_xent_fwd(None, 0, 512, 512, None, 512, None, 10, None, None, None, None, None, 0, None) == 0
    assert lib.tal_xent_rows_fwd(None, 4, 64, 64, None, None, 10, None, None, None, None, None, 0, None) == -1
    assert b"null pointer" in lib.tal_last_error()
    assert lib.tal_xent_lse_rows(None, 4, 10, None, None, None, None, None) == -1 and b"null pointer" in lib.tal_last_error()
    assert lib.tal_xent_lse_rows(None, 4, 0, None, None, None, None, None) == -1 and b"bad shape" in lib.tal_last_error()
    assert lib.tal_lm_xent_fwd(None, 4, 512, 512, None, 64, None, 10, None, None, None, None, None, 0, None) == -1
    assert b"no projection" in lib.tal_last_error()
    assert lib.tal_lm_xent_fwd(None, 4, 510, 512, None, 512, None, 10, None, None, None, None, None, 0, None) == -1


def test_the_two_options_enumerate():
    from tal_asrd_amd import _native as N
    lib = N.lib()
    names = []
    while lib.tal_option_name(len(names)):
        names.append(lib.tal_option_name(len(names)).decode())
    assert "xent_form" in names and "xent_grid" in names
    assert N.get_option("xent_form") == 0 and N.get_option("xent_grid") == 0
    try:
        N.set_option("xent_form", 2)
        N.set_option("xent_grid", 7)
        assert N.get_option("xent_form") == 2 and N.get_option("xent_grid") == 7
        assert lib.tal_set_option(b"xent_form", 3) == -1 and lib.tal_set_option(b"xent_grid", -1) == -1
        assert N.get_option("xent_form") == 2 and N.get_option("xent_grid") == 7
    finally:
        N.set_option("xent_form", 0)
        N.set_option("xent_grid", 0)


def test_no_cpu_fallback_and_the_public_methods_exist():
    from tal_asrd_amd import ASRModel, NativeError, ops
    from tal_asrd_amd.system import System
    with pytest.raises(NativeError):
        ops.xent_rows(torch.zeros(4, 64), torch.zeros(10, 64), None, torch.zeros(4, dtype=torch.long))
    with pytest.raises(NativeError):
        ops.xent_lse_rows(torch.zeros(4, 10), torch.zeros(4, dtype=torch.long))
    for cls, names in ((ASRModel, ("score",)), (System, ("score", "validation_step", "validation_end"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    # validation_end is the stack-and-mean of the reference (no device needed)
    s = System(model=None)
    out = s.validation_end([{"val_loss": torch.tensor(1.0), "val_lm_loss": torch.tensor(3.0)},
                            {"val_loss": torch.tensor(2.0), "val_lm_loss": torch.tensor(5.0)}])
    assert float(out["val_loss"]) == 1.5 and float(out["val_lm_loss"]) == 4.0 and out["log"]["val_loss"] is out["val_loss"]
