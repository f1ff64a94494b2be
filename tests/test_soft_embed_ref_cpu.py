"""CPU checks of the soft-embedding model and comparison (tests/_soft_embed_ref.py) and of the boundary of the new entry points: the
model against torch's float64 softmax and matmul, a plain fp32 evaluation inside the derived bound (bit-equal on the exact cases),
every wrong-model variant rejected by at least one case, the case table's claims, and the C ABI's exports, options and argument
checks (none of which needs a device)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _soft_embed_ref as R
from tests.conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tal_asrd.h")
SYMBOLS = ("tal_soft_embed_workspace_bytes", "tal_soft_embed_fwd", "tal_soft_embed_rows_workspace_bytes", "tal_soft_embed_rows",
           "tal_lm_soft_embed_workspace_bytes", "tal_lm_soft_embed_fwd")


def _refs(name):
    """the (aliased, separate) references of a case that exist"""
    return [r for r in R.build(name)[4:] if r is not None]


def _fp32(feat, W, b, V):
    """the operation in plain fp32 (torch CPU): what any correct fp32 kernel must be about as good as"""
    z = torch.from_numpy(feat) @ torch.from_numpy(W).T + torch.from_numpy(b)
    return (torch.softmax(z, dim=1) @ torch.from_numpy(V)).numpy(), torch.logsumexp(z, dim=1).numpy()


def test_the_model_is_softmax_times_values():
    feat, W, b, V, ra, rs = R.build("random-33-300-128")
    z = torch.from_numpy(feat).double() @ torch.from_numpy(W).double().T + torch.from_numpy(b).double()
    p = torch.softmax(z, dim=1)
    assert np.abs((p @ torch.from_numpy(V).double()).numpy() - rs.out).max() < 1e-12
    assert np.abs((p @ torch.from_numpy(W).double()).numpy() - ra.out).max() < 1e-12
    assert np.abs(torch.logsumexp(z, dim=1).numpy() - rs.lse).max() < 1e-12
    # masked columns add nothing: the model on the kept columns alone
    feat, W, b, V, ra, rs = R.build("masked-129-300-128-scattered")
    keep = np.isfinite(b)
    sub = R.make_ref(feat, W[keep], b[keep], V[keep])
    assert np.abs(sub.out - rs.out).max() < 1e-12 and np.abs(sub.lse - rs.lse).max() < 1e-12
    assert np.isfinite(rs.out).all() and np.isfinite(rs.tol).all()


def test_the_online_form_of_the_mutants_is_the_model_when_nothing_is_left_out():
    for name in ("order-129-300-128-rising", "order-129-300-128-rowdep", "masked-33-300-128-first", "random-129-127-64"):
        ref = _refs(name)[-1]
        out, lse = R._online(ref.z, ref.V)
        assert np.abs(out - ref.out).max() < 1e-12 and np.abs(lse - ref.lse).max() < 1e-10, name


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_a_plain_fp32_evaluation_is_within_the_bound(name):
    feat, W, b, V, ra, rs = R.build(name)
    E = W.shape[1]
    for ref, vals in ((ra, W), (rs, V)):
        if ref is None:
            continue
        out, lse = _fp32(np.ascontiguousarray(feat[:, :E]), W, b, vals)
        assert R.compare(ref, out, lse) == [], name
        assert R.error_ratio(ref, out) <= 1.0


@pytest.mark.parametrize("name", sorted(R.ROWS_CASES))
def test_rows_cases_in_plain_fp32(name):
    x, V, ref = R.build_rows(name)
    xt = torch.from_numpy(x)
    assert R.compare(ref, (torch.softmax(xt, dim=1) @ torch.from_numpy(V)).numpy(), torch.logsumexp(xt, dim=1).numpy()) == [], name


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_every_wrong_variant_fails_some_case(variant):
    failed = []
    for name in R.CASES:
        for ref in _refs(name):
            if variant == "keys_as_values" and not ref.separate:
                continue              # (values = W: the variant IS the model there)
            if R.compare(ref, *ref.wrong(variant)):
                failed.append(name)
    assert failed, "no case tells the model from the variant '%s'" % variant


def test_the_table_covers_what_it_claims():
    seen = [(c["E"], c["N"], c["M"]) for c in R.CASES.values() if c["kind"] == "random"]
    for E in R.FUSED_WIDTHS:
        for N in R.NS:
            assert any(e == E and n == N for e, n, _ in seen), (E, N)
        for M in R.MS:
            assert any(e == E and m == M for e, _, m in seen), (E, M)
    assert (128, 6008, 160) in seen
    assert any(c["N"] % 4 and c["N"] > 300 for c in R.CASES.values())
    assert any(c["E"] == 32 and c["D"] == 20 for c in R.CASES.values())
    assert any(c.get("ldf", c["E"]) > c["E"] for c in R.CASES.values())
    # one winner at columns 0, 127, 128, N - 1 and inside the ragged last tile; two and four equal winners in different tiles
    singles = {c["plants"][0] for c in R.CASES.values() if c["kind"] == "exact" and len(c["plants"]) == 1 and c["N"] == 300}
    assert {0, 127, 128, 299} <= singles and any(256 < s < 299 for s in singles)
    for n in (2, 4):
        assert any(c["kind"] == "exact" and len(c["plants"]) == n and len({p // 128 for p in c["plants"]}) >= 2 and
                   len({p // 64 for p in c["plants"]}) == n for c in R.CASES.values()), n
    ref = R.build("exact-129-300-128-four")[5]
    assert np.array_equal(ref.out[7], R.build("exact-129-300-128-four")[3][[3, 70, 130, 297]].astype(np.float64).mean(axis=0))
    # the four orders of the running maximum: where a left-to-right scan raises it
    def raises(name):
        z = _refs(name)[-1].z
        run = np.maximum.accumulate(z, axis=1)
        return [(run[:, c] > run[:, c - 1]).any() for c in range(64, z.shape[1], 64)], z
    up, _ = raises("order-129-300-128-rising")
    assert all(up)
    down, _ = raises("order-129-300-128-falling")
    assert not any(down)
    mid, z = raises("order-129-300-128-middle")
    assert mid[0] and mid[1] and not mid[-1] and (np.argmax(z, axis=1) // 64 == 2).all()
    _, z = raises("order-129-300-128-rowdep")
    peak = np.argmax(z, axis=1)
    assert np.array_equal(peak, (37 * np.arange(129)) % 300)
    assert all(len(set((peak[r0:r0 + 32] // 64).tolist())) >= 4 for r0 in range(0, 128, 32))      # per 32-row block: many tiles
    # masked: the first 128 columns as a whole; scattered ones on both sides of tile edges; every row keeps a finite column
    b = R.build("masked-33-300-128-first")[2]
    assert np.isinf(b[:128]).all() and np.isfinite(b[128:]).all()
    b = R.build("masked-129-300-128-scattered")[2]
    assert np.isinf(b[[0, 63, 64, 127, 299]]).all() and np.isfinite(b).sum() > 200


# ------------------------------------------------------------------ the boundary
def test_the_header_declares_the_entry_points_and_options():
    text = open(HEADER).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, text), name
    options = text[text.index("Process-wide behaviour switches"):text.index("int tal_set_option")]
    assert "soft_embed_form" in options and "soft_embed_grid" in options
    assert options.index("xent_form") < options.index("soft_embed_form")


def test_symbols_and_binding_table():
    from tal_asrd_amd import _native as N
    lib = N.lib()
    for name in SYMBOLS:
        assert name in N.SIGNATURES and hasattr(lib, name), name
    assert lib.tal_soft_embed_workspace_bytes(0, 10, 64, 64) == 0 and lib.tal_lm_soft_embed_workspace_bytes(4, 512, 64, 100, 100) == 0
    assert lib.tal_soft_embed_rows_workspace_bytes(300, 1001, 20) == (20 + 300) * 1004 * 4
    # widths without a fused form: the generic form's figure whatever the option
    assert lib.tal_soft_embed_workspace_bytes(300, 1001, 32, 20) == (20 + 300) * 1004 * 4
    try:
        N.set_option("soft_embed_form", 1)
        # the generic form: values^T and at most 64 MiB of probabilities at a pitch that is a multiple of 4
        assert lib.tal_soft_embed_workspace_bytes(300, 1001, 64, 64) == (64 + 300) * 1004 * 4
        assert lib.tal_soft_embed_workspace_bytes(1 << 20, 6008, 128, 128) <= (64 << 20) + 128 * 6008 * 4
        assert lib.tal_lm_soft_embed_workspace_bytes(8192, 512, 64, 16008, 10000) <= (64 << 20) + 64 * 6008 * 4 + 8192 * 64 * 4
    finally:
        N.set_option("soft_embed_form", 0)
    try:
        N.set_option("soft_embed_form", 2)
        # the fused form's partials: (max, sum, out[D]) per row and slot, far below the logits
        fused = lib.tal_soft_embed_workspace_bytes(44983, 6008, 128, 128)
        assert 44983 * 132 * 4 <= fused <= 44983 * 16 * 132 * 4 and fused < 44983 * 6008 * 4 // 8
    finally:
        N.set_option("soft_embed_form", 0)


def test_arguments_are_checked_before_any_launch():
    from tal_asrd_amd import _native as N
    import ctypes as C
    lib = N.lib()
    for M, ldf, E, n, D in ((-1, 64, 64, 10, 64), (4, 64, 0, 10, 64), (4, 64, 64, 0, 64), (4, 63, 64, 10, 64), (4, 64, 64, 10, 0)):
        assert lib.tal_soft_embed_fwd(None, M, ldf, E, None, None, n, None, D, None, None, None, 0, None) == -1, (M, ldf, E, n, D)
        assert b"bad shape" in lib.tal_last_error()
    assert lib.tal_soft_embed_fwd(None, 4, 64, 64, None, None, 10, None, 32, None, None, None, 0, None) == -1
    assert b"values == NULL" in lib.tal_last_error()
    assert lib.tal_soft_embed_fwd(None, 0, 64, 64, None, None, 10, None, 64, None, None, None, 0, None) == 0        # M == 0
    assert lib.tal_soft_embed_rows(None, 0, 10, None, 4, None, None, None, 0, None) == 0
    assert lib.tal_lm_soft_embed_fwd(None, 0, 512, 512, None, 512, None, 10, 3, None, None, None, 0, None) == 0
    assert lib.tal_soft_embed_fwd(None, 4, 64, 64, None, None, 10, None, 64, None, None, None, 0, None) == -1
    assert b"null pointer" in lib.tal_last_error()
    assert lib.tal_soft_embed_rows(None, 4, 10, None, 4, None, None, None, 0, None) == -1 and b"null pointer" in lib.tal_last_error()
    assert lib.tal_soft_embed_rows(None, 4, 0, None, 4, None, None, None, 0, None) == -1 and b"bad shape" in lib.tal_last_error()
    assert lib.tal_lm_soft_embed_fwd(None, 4, 512, 512, None, 64, None, 10, 3, None, None, None, 0, None) == -1
    assert b"no projection" in lib.tal_last_error()
    assert lib.tal_lm_soft_embed_fwd(None, 4, 512, 512, None, 512, None, 10, 10, None, None, None, 0, None) == -1
    assert b"col_begin" in lib.tal_last_error()
    # a short workspace is refused before anything is dereferenced or launched (the pointers are never followed), in every form
    p = C.c_void_p(4096)
    for form in (0, 1, 2):
        try:
            N.set_option("soft_embed_form", form)
            assert lib.tal_soft_embed_fwd(p, 4, 64, 64, p, None, 10, None, 64, p, None, p, 16, None) == -2, form
            assert b"workspace 16 <" in lib.tal_last_error()
            assert lib.tal_soft_embed_fwd(p, 4, 64, 64, p, None, 10, None, 64, p, None, None, 1 << 30, None) == -2, form
            assert lib.tal_lm_soft_embed_fwd(p, 4, 512, 512, p, 64, p, 100, 50, p, None, p, 4 * 64 * 4 + 16, None) == -2, form
        finally:
            N.set_option("soft_embed_form", 0)
    assert lib.tal_soft_embed_rows(p, 4, 10, p, 4, p, None, p, 16, None) == -2
    # the fused form where the shape does not allow it is an error, not a fallback
    try:
        N.set_option("soft_embed_form", 2)
        for E, D, ldf, feat in ((32, 32, 32, 4096), (128, 64, 128, 4096), (64, 64, 66, 4096), (64, 64, 64, 4100)):
            assert lib.tal_soft_embed_fwd(C.c_void_p(feat), 4, ldf, E, p, None, 10, p, D, p, None, p, 1 << 30, None) == -1, (E, D, ldf)
            assert b"fused form" in lib.tal_last_error()
    finally:
        N.set_option("soft_embed_form", 0)


def test_the_two_options_enumerate():
    from tal_asrd_amd import _native as N
    lib = N.lib()
    names = []
    while lib.tal_option_name(len(names)):
        names.append(lib.tal_option_name(len(names)).decode())
    assert "soft_embed_form" in names and "soft_embed_grid" in names
    assert N.get_option("soft_embed_form") == 0 and N.get_option("soft_embed_grid") == 0
    try:
        N.set_option("soft_embed_form", 2)
        N.set_option("soft_embed_grid", 7)
        assert N.get_option("soft_embed_form") == 2 and N.get_option("soft_embed_grid") == 7
        assert lib.tal_set_option(b"soft_embed_form", 3) == -1 and lib.tal_set_option(b"soft_embed_grid", -1) == -1
        assert N.get_option("soft_embed_form") == 2 and N.get_option("soft_embed_grid") == 7
    finally:
        N.set_option("soft_embed_form", 0)
        N.set_option("soft_embed_grid", 0)


def test_no_cpu_fallback_and_the_public_methods_exist():
    from tal_asrd_amd import ASRModel, NativeError, SDModel, ops
    from tal_asrd_amd.system import System
    with pytest.raises(NativeError):
        ops.soft_embed(torch.zeros(4, 64), torch.zeros(10, 64), None)
    with pytest.raises(NativeError):
        ops.soft_embed_rows(torch.zeros(4, 10), torch.zeros(10, 8))
    for cls, names in ((SDModel, ("speaker_soft_embeds", "speaker_soft_embeds_from_logmel")), (ASRModel, ("speaker_token_embeds",)),
                       (System, ("speaker_token_embeds",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
