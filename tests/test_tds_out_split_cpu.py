"""tal_tds_out_split on the host (no GPU): the form the TDS encoder driver's stage walk ends in, pinned on a table of descriptors,
flags, options and lengths.  The query is the driver's own walk with launching switched off (csrc/api.hip, tds_walk), so a row
here pins the decision chain of tal_tds_fwd as well; tests/test_gpu_tds_out_split.py ties the query to what a call records."""
import ctypes as C

import pytest

from tal_asrd_amd import _native as N

STOCK = (80, 800, 1120, 1440)
PTR = 4096          # any non-null, 16-byte aligned value: the query reads no weight


def _desc(depths=(2, 3, 6), channels=STOCK, groups=80, ksize=0, flags=N.TAL_TDS_OUT_SPLIT, fragments=True):
    d = N.TdsDesc()
    d.n_stages, d.groups, d.ksize, d.flags = len(depths), groups, ksize, flags
    for i, c in enumerate(channels[:len(depths) + 1]):
        d.channels[i] = c
    for i, n in enumerate(depths):
        d.depths[i] = n
        d.down_w[i] = d.down_b[i] = PTR
        if fragments and i > 0:
            d.down_w_frag[i] = PTR
        for j in range(n):
            bw = d.blocks[i][j]
            bw.conv_w = bw.conv_b = bw.fc0_w = bw.fc0_b = bw.fc3_w = bw.fc3_b = PTR
            bw.fc0_w_split = bw.fc3_w_split = PTR
            if fragments:
                bw.conv_w_frag = PTR
    return d


def _without(d, what, i, j=0):
    if what == "down_w_frag":
        d.down_w_frag[i] = None
    else:
        setattr(d.blocks[i][j], what, None)
    return d


BOTH = N.TAL_TDS_OUT_SPLIT | N.TAL_TDS_EXACT_F32
# (id, descriptor, options, B, T, expected).  Stock stack, one item: T = 1161 -> 571 -> 276 -> 128 frames, T = 1165 -> 573 -> 277 -> 129; the
# last stage runs all-split from 129 rows on (M > 128).
TABLE = [
    ("stock_long", lambda: _desc(), {}, 1, 360000, 1),
    ("stock_129_rows", lambda: _desc(), {}, 1, 1165, 1),
    ("stock_128_rows", lambda: _desc(), {}, 1, 1161, 0),
    ("two_items_130_rows", lambda: _desc(), {}, 2, 653, 1),          # 653 -> 317 -> 149 -> 65 frames per item
    ("two_items_128_rows", lambda: _desc(), {}, 2, 645, 0),          # 645 -> 313 -> 147 -> 64
    ("no_flag", lambda: _desc(flags=0), {}, 1, 360000, 0),
    ("exact_flag", lambda: _desc(flags=BOTH), {}, 1, 360000, 0),
    ("option_exact", lambda: _desc(), {"tds_exact_f32": 1}, 1, 360000, 0),
    ("option_fp32_activations", lambda: _desc(), {"tds_fp32_activations": 1}, 1, 360000, 0),
    ("no_fc3_split_in_last_stage", lambda: _without(_desc(), "fc3_w_split", 2, 5), {}, 1, 360000, 0),
    ("no_conv_frag_in_first_stage", lambda: _without(_desc(), "conv_w_frag", 0, 1), {}, 1, 360000, 1),   # the last stage alone decides
    ("no_down_frag_2", lambda: _without(_desc(), "down_w_frag", 2), {}, 1, 360000, 0),  # 14 -> 18 per group: no other split-writing kernel
    ("no_down_frag_1", lambda: _without(_desc(), "down_w_frag", 1), {}, 1, 360000, 1),
    ("last_stage_without_blocks", lambda: _desc((2, 3, 0)), {}, 1, 360000, 0),
    ("middle_stage_without_blocks", lambda: _desc((2, 0, 1)), {}, 1, 360000, 1),
    ("one_stage", lambda: _desc((2,)), {}, 1, 360000, 1),              # the 1 -> 10 channel kernel writes the split form
    ("one_stage_c1_generic", lambda: _desc((2,)), {"gconv_c1_generic": 1}, 1, 360000, 0),
    ("eight_groups", lambda: _desc(channels=(8, 80, 112, 144), groups=8), {}, 1, 360000, 0),     # widths that are no multiple of 160
    ("ksize_15", lambda: _desc(ksize=15, fragments=False), {}, 1, 360000, 0),
    ("ksize_21_general", lambda: _desc(ksize=21), {"gconv_general": 1}, 1, 360000, 0),
    ("too_short", lambda: _desc(), {}, 1, 140, 0),
]


@pytest.mark.parametrize("name,make,opts,B,T,want", TABLE, ids=[r[0] for r in TABLE])
def test_out_split_table(name, make, opts, B, T, want):
    lib = N.lib()
    d = make()
    saved = {k: N.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            N.set_option(k, v)
        got = lib.tal_tds_out_split(C.byref(d), B, T)
    finally:
        for k, v in saved.items():
            N.set_option(k, v)
    assert got == want, (name, got)
    assert {k: N.get_option(k) for k in opts} == saved


def test_table_cannot_pass_on_a_constant_answer():
    assert sum(r[5] for r in TABLE) >= 4 and sum(1 - r[5] for r in TABLE) >= 4
