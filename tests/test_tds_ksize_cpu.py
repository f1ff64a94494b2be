"""TDS / TDSBlock at kernel sizes other than 21, host side (no GPU): constructors and their limits, state-dict layout against the
reference's, the descriptor field, the C and Python length / halo arithmetic, the descriptor checks, and the float64 restatement
(tests/_tds_ksize_ref.py) against the fixtures recorded from the reference (tests/golden/make_golden_tds_ksize.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tal_asrd_amd import _native as N, tiling
from tal_asrd_amd.models import TDS, TDSBlock
from tests import _tds_ksize_ref as R
from tests.conftest import GOLDEN, golden

SIZES, DEPTHS = [80, 800, 1120, 1440], [2, 3, 6]


@pytest.mark.parametrize("k", [1, 3, 15, 21, 31, 63])
def test_constructors_accept_odd_kernel_sizes(k):
    m = TDS(80, SIZES, DEPTHS, kernel_size=k)
    assert m.kernel_size == k
    assert m.blocks[0][0].kernel_size == (k,) and m.blocks[2][1][5].conv[0].kernel_size == (k,)
    assert m.blocks[1][1][0].conv[0].padding == (k // 2,)
    assert TDSBlock(32, k, 8).conv[0].kernel_size == (k,)


def test_even_kernel_size_without_blocks_is_a_resize_only_stack():
    m = TDS(8, [8, 16, 24, 32], [0, 0, 0], kernel_size=8)
    assert m.kernel_size == 8 and m.blocks[2][0].kernel_size == (8,) and len(m.blocks[2][1]) == 0


@pytest.mark.parametrize("k", [0, 64, -3])
def test_kernel_size_out_of_range_raises(k):
    with pytest.raises(N.NativeError, match=r"kernel_size=%d outside 1\.\.63" % k):
        TDS(80, SIZES, DEPTHS, kernel_size=k)
    with pytest.raises(N.NativeError, match=r"kernel_size=%d outside 1\.\.63" % k):
        TDSBlock(32, k, 8)


@pytest.mark.parametrize("k", [2, 8, 20])
def test_even_kernel_size_with_blocks_raises(k):
    with pytest.raises(N.NativeError, match=r"kernel_size=%d is even: the reference's TDSBlock residual add fails.*T \+ 1 frames" % k):
        TDSBlock(32, k, 8)
    with pytest.raises(N.NativeError, match="residual add fails"):
        TDS(8, [8, 16, 24, 32], [0, 1, 0], kernel_size=k)


@pytest.mark.parametrize("k", [3, 15])
def test_state_dict_keys_and_shapes_match_the_reference(k):
    keys = json.load(open(os.path.join(GOLDEN, "tds_ksize_keys.json")))
    ours = [[n, list(v.shape)] for n, v in TDS(80, SIZES, DEPTHS, kernel_size=k).state_dict().items()]
    assert ours == keys["TDS_k%d" % k]
    ours = [[n, list(v.shape)] for n, v in TDSBlock(32, k, 8).state_dict().items()]
    assert ours == keys["TDSBlock_k%d" % k]


def test_descriptor_ksize_field_takes_the_old_padding_slot():
    # the field that follows `flags` and ends the struct (formerly _pad2): the layout is unchanged
    assert N.TdsDesc.ksize.offset == N.TdsDesc.flags.offset + 4
    assert C.sizeof(N.TdsDesc) == N.TdsDesc.flags.offset + 8
    assert N.TdsDesc.ksize.size == 4


def _desc(depths, ksize, groups=80):
    d = N.TdsDesc()
    d.n_stages, d.groups, d.ksize = len(depths), groups, ksize
    for i in range(len(depths) + 1):
        d.channels[i] = groups * (1 if i == 0 else 8 + 2 * i)
    for i, v in enumerate(depths):
        d.depths[i] = v
    return d


@pytest.mark.parametrize("ksize", [0, 21, 3, 15, 31])
def test_host_arithmetic_agrees_between_c_and_python(ksize):
    lib = N.lib()
    k = ksize or 21
    for depths in ((2, 3, 6), (1, 1, 2), (0, 4, 1), (3,), (0, 0)):
        d = _desc(depths, ksize)
        for T in (0, 1, k - 1, k, k + 1, 141, 1000, 30001, 360001):
            assert lib.tal_tds_out_len(C.byref(d), T) == tiling.tds_out_len(T, len(depths), k), (depths, T)
        left, right, stride = C.c_int64(), C.c_int64(), C.c_int64()
        assert lib.tal_tds_halo(C.byref(d), C.byref(left), C.byref(right), C.byref(stride)) == 0, N.lib().tal_last_error()
        assert (left.value, right.value, stride.value) == tiling.receptive_halo(depths, k), depths
        if depths == (2, 3, 6):
            assert (left.value, right.value, stride.value) == {21: (640, 780, 8), 15: (448, 546, 8)}.get(k, (left.value, right.value, 8))
        # the tiled plan sizes its slices from the same halo
        T, tile = 30001, 512
        plan = tiling.plan_tiles(T, tile, depths, kernel_size=k)
        if plan:
            longest = max(t.in_stop - t.in_start for t in plan)
            need = lib.tal_tds_tiled_workspace_bytes(C.byref(d), T, tile)
            assert need >= lib.tal_tds_workspace_bytes(C.byref(d), 1, longest) + 64
            for t in plan:
                assert tiling.tds_out_len(t.in_stop - t.in_start, len(depths), k) >= t.skip + (t.out_stop - t.out_start)
    assert tiling.receptive_halo((2, 3, 6), 15) == (448, 546, 8)


def test_python_defaults_keep_k21():
    assert tiling.tds_out_len(141) == 1 == tiling.tds_out_len(141, 3, 21)
    assert tiling.plan_tiles(30001, 256) == tiling.plan_tiles(30001, 256, (2, 3, 6), kernel_size=21)
    assert tiling.plan_tiles(30001, 256, (2, 3, 6), kernel_size=15) != tiling.plan_tiles(30001, 256)


def test_too_short_message_names_the_kernel_size():
    lib = N.lib()
    d = _desc((2, 3, 6), 15)
    assert lib.tal_tds_out_len(C.byref(d), 20) == 0 and lib.tal_tds_out_len(C.byref(d), 99) == 1     # 99 -> 43 -> 15 -> 1
    rc = lib.tal_tds_fwd(C.byref(d), 16, 1, 20, 16, 16, 1 << 20, None)
    assert rc == -1 and b"k=15" in lib.tal_last_error()


def test_check_desc_rejects_bad_ksize_and_fragments():
    lib = N.lib()
    out = C.c_int64()
    for bad in (-1, 64, 100):
        d = _desc((2, 3, 6), bad)
        assert lib.tal_tds_halo(C.byref(d), C.byref(out), None, None) == -1
        assert b"ksize" in lib.tal_last_error()
    d = _desc((2, 0, 1), 8)                          # even k: only where a stage has TDSBlocks
    assert lib.tal_tds_halo(C.byref(d), C.byref(out), None, None) == -1 and b"ksize=8 is even" in lib.tal_last_error()
    assert lib.tal_tds_halo(C.byref(_desc((0, 0, 0), 8)), C.byref(out), None, None) == 0
    d = _desc((2, 3, 6), 15)
    d.down_w_frag[1] = 4096
    assert lib.tal_tds_halo(C.byref(d), C.byref(out), None, None) == -1 and b"down_w_frag[1]" in lib.tal_last_error()
    d = _desc((2, 3, 6), 15)
    d.blocks[2][4].conv_w_frag = 4096
    assert lib.tal_tds_halo(C.byref(d), C.byref(out), None, None) == -1 and b"conv_w_frag" in lib.tal_last_error()
    for ok in (0, 21):                               # fragments belong to the k = 21 descriptor
        d = _desc((2, 3, 6), ok)
        d.down_w_frag[1] = 4096
        d.blocks[2][4].conv_w_frag = 4096
        assert lib.tal_tds_halo(C.byref(d), C.byref(out), None, None) == 0
    # a k != 21 descriptor has no premean / split-output form
    d = _desc((2, 3, 6), 15)
    assert lib.tal_tds_premean_ok(C.byref(d), 4096) == 0
    d.flags = N.TAL_TDS_OUT_SPLIT
    assert lib.tal_tds_out_split(C.byref(d), 1, 360000) == 0


def test_pack_weight_accepts_the_kernel_size_range():
    lib = N.lib()
    for k in (0, 64):
        assert lib.tal_pack_gconv_weight(16, 16, 8, 1, k, 8, None) == -1
        assert b"kernel size" in lib.tal_last_error()


def test_version_and_option():
    lib = N.lib()
    assert lib.tal_version() == 501
    names = []
    i = 0
    while lib.tal_option_name(i):
        names.append(lib.tal_option_name(i))
        i += 1
    assert b"gconv_general" in names
    v = C.c_int(-1)
    assert lib.tal_get_option(b"gconv_general", C.byref(v)) == 0 and v.value == 0


def _small(k, depths):
    return TDS(input_size=8, sizes=[8, 16, 24, 32], depths=depths, kernel_size=k)


@pytest.mark.parametrize("k,depths", [(3, [1, 1, 2]), (11, [1, 1, 2]), (31, [1, 1, 2]), (8, [0, 0, 0])])
def test_float64_restatement_reproduces_the_reference_tds(k, depths):
    g = golden("tds_ksize")
    sd = R.synth_weights(_small(k, depths), "tds_k%d." % k)
    x = torch.from_numpy(g["tds_k%d_x" % k])
    y = R.tds(x, sd, 8, depths, k, torch.float64).numpy()
    ref = g["tds_k%d_y" % k]
    assert y.shape == ref.shape
    np.testing.assert_allclose(y, ref, rtol=0, atol=2e-5 * max(1.0, float(np.abs(ref).max())))


@pytest.mark.parametrize("k", [5, 15])
def test_float64_restatement_reproduces_the_reference_block(k):
    g = golden("tds_ksize")
    sd = R.synth_weights(TDSBlock(32, k, 8), "block_k%d." % k)
    x = torch.from_numpy(g["block_k%d_x" % k])
    y = R.block(x, sd, "", 8, k, torch.float64).numpy()
    ref = g["block_k%d_y" % k]
    assert y.shape == ref.shape == x.shape
    np.testing.assert_allclose(y, ref, rtol=0, atol=2e-5 * max(1.0, float(np.abs(ref).max())))
