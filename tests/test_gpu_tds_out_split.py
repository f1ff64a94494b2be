"""The output form of an encoder call (GPU): with TAL_TDS_OUT_SPLIT set, word 1 of the call's status block -- written by tal_tds_fwd
from its walk over the stages without launches -- equals tal_tds_out_split's answer (the same walk) and the form expected for the
shape, on both sides of the last stage's 128 | 129 rows; the output, read as hi + lo * 2^-11 where it is split, agrees with the same
call on the exact fp32 kernels within the element-wise bound of tests/test_gpu_fp16x3_range.py (_encoder_bound)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _fp16x3_ref as R
from tests.conftest import has_gpu
from tests.test_gpu_fp16x3_range import _Tracer, _encoder_bound, dev

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

# one item: T = 1161 -> 571 -> 276 -> 128 frames, T = 1165 -> 573 -> 277 -> 129; the last stage runs all-split above 128 rows
SHAPES = [(1, 1161), (1, 1165), (2, 1165)]
SPLIT_BY_DEFAULT = {(1, 1161): 0, (1, 1165): 1, (2, 1165): 1}
SETTINGS = ["default", "tds_fp32_activations", "exact_flag"]


class _Stack:
    """TDS(80, [80, 800, 1120, 1440], [1, 1, 1]) with the range tests' random weights; per shape the input, the float64 output,
    its bound and the exact-mode call's output, each computed once."""

    def __init__(self):
        self.tracer = _Tracer()
        self.p = self.tracer.base
        self.tracer.load(self.p)
        self.cases = {}

    def call(self, x, flags):
        """tal_tds_fwd with `flags` -> (y tensor, range word, form word)"""
        from tal_asrd_amd import _native as N, ops
        lib = N.lib()
        B, T, _ = x.shape
        desc = N.TdsDesc.from_buffer_copy(self.tracer.tds._descriptor())
        desc.flags |= flags
        y = torch.empty(B, lib.tal_tds_out_len(C.byref(desc), T), 1440, dtype=torch.float32, device=dev())
        nws = lib.tal_tds_workspace_bytes(C.byref(desc), B, T)
        ws = ops._ws(nws, dev())
        N.check(ops._tds_call(lib, desc, x.to(dev()), None, B, T, y, ws, nws), "tal_tds_fwd")
        torch.cuda.synchronize()
        off = lib.tal_tds_status_offset(C.byref(desc), B, T)
        flag, form = ws[off:off + 8].view(torch.int32).tolist()
        return y, flag, form, lib.tal_tds_out_split(C.byref(desc), B, T)

    def case(self, B, T):
        from tal_asrd_amd import _native as N
        if (B, T) not in self.cases:
            x = torch.randn(B, T, 80, generator=torch.Generator().manual_seed(100 * B + T))
            want = self.tracer.activations64(self.p, x)["s2.fc3"]
            y, _, form, _ = self.call(x, N.TAL_TDS_OUT_SPLIT | N.TAL_TDS_EXACT_F32)
            assert form == 0
            self.cases[(B, T)] = (x, _encoder_bound(self.tracer, self.p, x, want), y.cpu().double().numpy())
        return self.cases[(B, T)]


@pytest.fixture(scope="module")
def stack():
    return _Stack()


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("B,T", SHAPES)
def test_recorded_form_is_the_predicted_form_and_the_values_agree(stack, B, T, setting):
    from tal_asrd_amd import _native as N
    x, bound, exact = stack.case(B, T)
    opts = {"tds_fp32_activations": 1} if setting == "tds_fp32_activations" else {}
    flags = N.TAL_TDS_OUT_SPLIT | (N.TAL_TDS_EXACT_F32 if setting == "exact_flag" else 0)
    expected = SPLIT_BY_DEFAULT[(B, T)] if setting == "default" else 0
    saved = {k: N.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            N.set_option(k, v)
        y, flag, form, predicted = stack.call(x, flags)
    finally:
        for k, v in saved.items():
            N.set_option(k, v)
    assert form == predicted == expected, (setting, B, T, form, predicted)
    assert flag == 0
    rows = exact.shape[0] * exact.shape[1]
    if form:
        got = R.decode_rows(y.cpu().numpy().view(np.uint16), rows, 1440).reshape(exact.shape)
    else:
        got = y.cpu().double().numpy()
    err = np.abs(got - exact)
    print("tds out form %s B=%d T=%d: form %d, max err / bound %.3f" % (setting, B, T, form, float((err / bound).max())))
    assert bool((err <= bound).all()), (setting, B, T, float((err / bound).max()))
