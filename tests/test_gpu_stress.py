"""Seeded random-shape sweeps of the kernels against float64 host references (GPU): tile-boundary rows, ragged
columns, K tails, guard rows behind every output, short / odd time axes."""
import numpy as np
import pytest
import torch

from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]


def dev():
    return torch.device("cuda:0")


def _linear_case(rng, M, N, K, mode):
    from tal_asrd_amd import ops
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / max(K, 1) ** 0.5
    b = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    guard = 3
    yfull = torch.full((M + guard, N), 777.0, device=dev())
    y = ops.linear(x.to(dev()), w.to(dev()), b.to(dev()), mode=mode, res=res.to(dev()) if mode == 2 else None, alpha=0.3,
                   out=yfull[:M])
    torch.cuda.synchronize()
    ref = x.double() @ w.double().t() + b.double()
    if mode == 1:
        ref = ref.clamp_min(0)
    if mode == 2:
        ref = res.double() + 0.3 * ref
    if mode == 3:
        ref = 0.3 * ref
    assert bool((yfull[M:] == 777.0).all()), (M, N, K, mode)
    err = float((y.cpu().double() - ref).abs().max()) if M else 0.0
    assert err < 2e-5 * max(1.0, K ** 0.5 / 8), (M, N, K, mode, err)


def test_linear_random_shapes():
    rng = np.random.default_rng(2024)
    for _ in range(40):                                   # small problems: every kernel of the small-M family
        M = int(rng.choice([1, 2, 31, 32, 33, 63, 64, 65, 127, 200, 511, 512]))
        N = int(rng.choice([1, 4, 31, 32, 33, 100, 128, 160, 161, 512, 2048]))
        K = int(rng.choice([4, 8, 28, 32, 36, 60, 64, 68, 128, 132, 512, 516, 2048]))
        _linear_case(rng, M, N, K, int(rng.integers(0, 4)))
    for _ in range(24):                                   # large problems: the 128 x 160 tile, ragged everything
        M = int(rng.choice([513, 640, 641, 767, 1000, 4097, 66000 + int(rng.integers(0, 300))]))
        N = int(rng.choice([32, 159, 160, 161, 320, 800]))
        K = int(rng.choice([32, 64, 96, 100, 256, 288, 800]))
        _linear_case(rng, M, N, K, int(rng.integers(0, 4)))


def test_gconv_random_shapes():
    from tal_asrd_amd import ops
    rng = np.random.default_rng(7)
    for _ in range(12):
        cg = int(rng.choice([10, 14, 18, 4]))
        G = 80 if cg != 4 else int(rng.choice([2, 8]))
        T = int(rng.choice([1, 5, 21, 63, 64, 255, 256, 257, 300, 513]))
        B = int(rng.integers(1, 3))
        g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
        x = torch.randn(B, G * cg, T, generator=g)
        w = torch.randn(G * cg, cg, 21, generator=g) / (21 * cg) ** 0.5
        b = torch.randn(G * cg, generator=g)
        ref = x.double() + 0.25 * torch.relu(torch.nn.functional.conv1d(x.double(), w.double(), b.double(), padding=10, groups=G))
        wp = ops.pack_gconv_weight(w.to(dev()), G)
        y = ops.gconv_res(x.permute(0, 2, 1).contiguous().to(dev()), wp, b.to(dev()), 0.25, G)
        np.testing.assert_allclose(y.cpu().double().numpy(), ref.permute(0, 2, 1).numpy(), atol=2e-5, rtol=1e-5,
                                   err_msg=str((cg, G, T, B)))
    for _ in range(10):
        cig, cog = [(1, 10), (10, 14), (14, 18), (2, 3)][int(rng.integers(0, 4))]
        G = 80 if cig != 2 else 8
        T = int(rng.choice([21, 22, 23, 64, 277, 300, 511, 1000]))
        B = int(rng.integers(1, 3))
        g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
        x = torch.randn(B, G * cig, T, generator=g)
        w = torch.randn(G * cog, cig, 21, generator=g) / (21 * cig) ** 0.5
        b = torch.randn(G * cog, generator=g)
        ref = torch.nn.functional.conv1d(x.double(), w.double(), b.double(), stride=2, groups=G).permute(0, 2, 1)
        wp = ops.pack_gconv_weight(w.to(dev()), G)
        y = ops.gconv_s2(x.permute(0, 2, 1).contiguous().to(dev()), wp, b.to(dev()), G * cog, G)
        np.testing.assert_allclose(y.cpu().double().numpy(), ref.numpy(), atol=2e-5, rtol=1e-5, err_msg=str((cig, cog, T, B)))


def test_gconv_f16x3_random_shapes():
    """matrix-core grouped convs (TDSBlock conv with fused residual, stride-2 resize convs) on odd time axes: tile and
    block boundaries of the 256- / 128-step tiles, inputs shorter than the halo, two batch items, guard rows (every call reads x
    from between NaN bands and writes between bands of 0x5A, which guarded_f16x3 wants back untouched)."""
    from tal_asrd_amd import ops
    from tests.test_gpu_gconv_guard import guarded_f16x3
    rng = np.random.default_rng(23)
    G = 80
    for _ in range(12):
        cg = int(rng.choice([10, 14, 18]))
        T = int(rng.choice([1, 2, 9, 10, 11, 15, 16, 17, 63, 255, 256, 257, 271, 300, 513, 777]))
        B = int(rng.integers(1, 3))
        g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
        x = torch.randn(B, G * cg, T, generator=g) * 3.0
        w = torch.randn(G * cg, cg, 21, generator=g) / (21 * cg) ** 0.5
        b = torch.randn(G * cg, generator=g)
        ref = x.double() + 0.4 * torch.relu(torch.nn.functional.conv1d(x.double(), w.double(), b.double(), padding=10, groups=G))
        wf = ops.pack_gconv_f16x3_weight(w.to(dev()), G)
        y = guarded_f16x3(x.permute(0, 2, 1).contiguous().to(dev()), wf, b.to(dev()), G, alpha=0.4)
        np.testing.assert_allclose(y.cpu().double().numpy(), ref.permute(0, 2, 1).numpy(), atol=3e-5, rtol=1e-5,
                                   err_msg=str((cg, T, B)))
    for _ in range(10):
        cig, cog = [(10, 14), (14, 18)][int(rng.integers(0, 2))]
        T = int(rng.choice([21, 22, 23, 24, 53, 54, 275, 276, 277, 278, 300, 511, 531, 1000]))
        B = int(rng.integers(1, 3))
        g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
        x = torch.randn(B, G * cig, T, generator=g) * 3.0
        w = torch.randn(G * cog, cig, 21, generator=g) / (21 * cig) ** 0.5
        b = torch.randn(G * cog, generator=g)
        ref = torch.nn.functional.conv1d(x.double(), w.double(), b.double(), stride=2, groups=G).permute(0, 2, 1)
        wf = ops.pack_gconv_f16x3_weight(w.to(dev()), G, stride=2)
        y = guarded_f16x3(x.permute(0, 2, 1).contiguous().to(dev()), wf, b.to(dev()), G, c_out=G * cog)
        np.testing.assert_allclose(y.cpu().double().numpy(), ref.numpy(), atol=3e-5, rtol=1e-5, err_msg=str((cig, cog, T, B)))


def _unsplit(buf, rows, C):
    """hi / lo split form (per row and 32-channel block: 32 hi halves, 32 lo halves) -> float64 [rows, C]"""
    h = buf.view(torch.float16).view(rows, C // 32, 2, 32).double()
    return (h[:, :, 0] + h[:, :, 1] / 2048.0).reshape(rows, C)


def test_gconv_split_form_random_shapes():
    """the grouped convs on activations that live in the hi / lo split form (input and output; the output tile is staged
    through the dead rows of the LDS slab and leaves along rows): odd time axes around the 16-step blocks and the 256- /
    128-step tiles, two batch items, every channel width."""
    from tal_asrd_amd import ops
    rng = np.random.default_rng(41)
    G = 80
    for _ in range(12):
        cg = int(rng.choice([10, 14, 18]))
        T = int(rng.choice([1, 15, 16, 17, 255, 256, 257, 271, 300, 513, 777, 1031]))
        B = int(rng.integers(1, 3))
        C = G * cg
        g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
        x = torch.randn(B, T, C, generator=g) * 3.0
        w = torch.randn(C, cg, 21, generator=g) / (21 * cg) ** 0.5
        b = torch.randn(C, generator=g)
        xs = ops.split_f16x3(x.reshape(B * T, C).to(dev()))
        xq = _unsplit(xs, B * T, C).reshape(B, T, C).cpu()          # what the kernel sees: x to 22 mantissa bits
        ref = xq + 0.4 * torch.relu(torch.nn.functional.conv1d(xq.permute(0, 2, 1), w.double(), b.double(), padding=10, groups=G)).permute(0, 2, 1)
        wf = ops.pack_gconv_f16x3_weight(w.to(dev()), G)
        ys = ops.gconv_res_split(xs, (B, T, C), wf, b.to(dev()), 0.4, G)
        got = _unsplit(ys, B * T, C).reshape(B, T, C).cpu()
        np.testing.assert_allclose(got.numpy(), ref.numpy(), atol=3e-5, rtol=1e-5, err_msg=str((cg, T, B)))
    for _ in range(10):
        cig, cog = [(10, 14), (14, 18)][int(rng.integers(0, 2))]
        T = int(rng.choice([21, 22, 23, 53, 275, 276, 277, 300, 511, 531, 1000]))
        B = int(rng.integers(1, 3))
        g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
        x = torch.randn(B, T, G * cig, generator=g) * 3.0
        w = torch.randn(G * cog, cig, 21, generator=g) / (21 * cig) ** 0.5
        b = torch.randn(G * cog, generator=g)
        xs = ops.split_f16x3(x.reshape(B * T, G * cig).to(dev()))
        xq = _unsplit(xs, B * T, G * cig).reshape(B, T, G * cig).cpu()
        ref = torch.nn.functional.conv1d(xq.permute(0, 2, 1), w.double(), b.double(), stride=2, groups=G).permute(0, 2, 1)
        T_out = ref.shape[1]
        wf = ops.pack_gconv_f16x3_weight(w.to(dev()), G, stride=2)
        ys = ops.gconv_s2_split(xs, (B, T, G * cig), True, wf, b.to(dev()), G * cog, G)
        got = _unsplit(ys, B * T_out, G * cog).reshape(B, T_out, G * cog).cpu()
        np.testing.assert_allclose(got.numpy(), ref.numpy(), atol=3e-5, rtol=1e-5, err_msg=str((cig, cog, T, B)))


def test_first_resize_conv_channel_major():
    """the 1 -> 10 channels-per-group conv (channel-major lanes, coalesced stores) against float64, incl. the shortest input."""
    from tal_asrd_amd import ops
    G = 80
    g = torch.Generator().manual_seed(99)
    for T, B in ((21, 1), (533, 2), (1000, 1)):
        x = torch.randn(B, T, G, generator=g).to(dev())
        w = torch.randn(G * 10, 1, 21, generator=g).to(dev())
        b = torch.randn(G * 10, generator=g).to(dev())
        wp = ops.pack_gconv_weight(w, G)
        y = ops.gconv_s2(x, wp, b, G * 10, G)
        ref = torch.nn.functional.conv1d(x.cpu().double().permute(0, 2, 1), w.cpu().double(), b.cpu().double(), stride=2, groups=G).permute(0, 2, 1)
        np.testing.assert_allclose(y.cpu().double().numpy(), ref.numpy(), atol=2e-5, rtol=1e-5)


def test_logmel_random_lengths():
    from oracle import tal_oracle as O
    from tal_asrd_amd import LogMelSpec
    rng = np.random.default_rng(11)
    m = LogMelSpec().to(dev())
    for _ in range(10):
        B = int(rng.integers(1, 4))
        L = int(rng.choice([201, 400, 401, 1599, 1600, 1601, 5120, 5121, 16000 + int(rng.integers(0, 200)), 48000]))
        audio = (rng.standard_normal((B, L)) * 0.1).astype(np.float32)
        got = m(torch.from_numpy(audio).to(dev())).cpu().numpy()
        assert got.shape == (B, 1 + L // 160, 80)
        np.testing.assert_allclose(got, O.logmel_f64(audio), atol=2e-4, rtol=0, err_msg=str((B, L)))


@pytest.mark.parametrize("M", [100, 512])
@pytest.mark.parametrize("S", [130, 160, 161, 225])
def test_sd_head_fused_argmax_partial_slots(M, S):
    """Small-M fused arg-max: the 32 x 128 tile kernel writes 4 partial slots per 128-column tile, so the partial row
    must hold 4 * ceil(S / 128) of them (S % 128 in [1, 96] used to overrun a ceil(S / 32)-wide row)."""
    from tal_asrd_amd import ops
    g = torch.Generator().manual_seed(1000 * M + S)
    x = torch.randn(M, 96, generator=g).to(dev())
    we = (torch.randn(128, 96, generator=g) / 10).to(dev())
    be = torch.randn(128, generator=g).to(dev())
    wl = (torch.randn(S, 128, generator=g) / 11).to(dev())
    bl = torch.randn(S, generator=g).to(dev())
    _, logits, ids_ref = ops.sd_head(x, we, be, wl, bl, want_logits=True, want_ids=True)
    _, _, ids = ops.sd_head(x, we, be, wl, bl, want_logits=False, want_ids=True)
    assert torch.equal(ids, ids_ref)
    assert torch.equal(ids.long().cpu(), logits.argmax(-1).cpu())


def test_sd_head_random_shapes():
    from tal_asrd_amd import ops
    rng = np.random.default_rng(5)
    for _ in range(8):
        M = int(rng.choice([1, 100, 513, 4000, 33000 + int(rng.integers(0, 500))]))
        S = int(rng.choice([160, 161, 1000, 6008]))
        g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
        x = torch.randn(M, 96, generator=g).to(dev())
        we = (torch.randn(128, 96, generator=g) / 10).to(dev())
        be = torch.randn(128, generator=g).to(dev())
        wl = (torch.randn(S, 128, generator=g) / 11).to(dev())
        bl = torch.randn(S, generator=g).to(dev())
        _, logits, ids_ref = ops.sd_head(x, we, be, wl, bl, want_logits=True, want_ids=True)
        _, _, ids = ops.sd_head(x, we, be, wl, bl, want_logits=False, want_ids=True)
        assert torch.equal(ids, ids_ref), (M, S)
        assert torch.equal(ids.long().cpu(), logits.argmax(-1).cpu()), (M, S)


@pytest.mark.range_fallback
def test_fp16_range_guard_routes_to_exact_kernels():
    """The fp16x3 form carries fp32 activations as two fp16 halves (|x| <= 65504).  A TDSBlock fed with activations ~1e5
    must not silently degrade: the kernels raise the status word, the call is re-run on the exact fp32-input kernels
    and matches float64 to the fp32 path's tolerance; in-range input must not trigger the fallback."""
    from tal_asrd_amd import TDS, ops, synth
    torch.manual_seed(3)
    tds = TDS(80, [80, 800], [1])                     # one stride-2 conv + one TDSBlock at 10 channels per group
    sd = synth.fill_state_dict({"g." + k: tuple(v.shape) for k, v in tds.state_dict().items()})
    own = tds.state_dict()
    for k in own:
        own[k] = torch.from_numpy(sd["g." + k].copy())
    tds.load_state_dict(own)
    tds64 = torch.nn.Sequential()                     # float64 reference of the same layers on the CPU
    conv0 = torch.nn.Conv1d(80, 800, 21, stride=2, groups=80).double()
    blk_conv = torch.nn.Conv1d(800, 800, 21, groups=80, padding=10).double()
    fc0 = torch.nn.Conv1d(800, 800, 1).double()
    fc3 = torch.nn.Conv1d(800, 800, 1).double()
    with torch.no_grad():
        conv0.weight.copy_(own["blocks.0.0.weight"]); conv0.bias.copy_(own["blocks.0.0.bias"])
        blk_conv.weight.copy_(own["blocks.0.1.0.conv.0.weight"]); blk_conv.bias.copy_(own["blocks.0.1.0.conv.0.bias"])
        fc0.weight.copy_(own["blocks.0.1.0.fc.0.weight"]); fc0.bias.copy_(own["blocks.0.1.0.fc.0.bias"])
        fc3.weight.copy_(own["blocks.0.1.0.fc.3.weight"]); fc3.bias.copy_(own["blocks.0.1.0.fc.3.bias"])
    rw = float(own["blocks.0.1.0.resweight"])

    def ref(x):
        with torch.no_grad():
            a = conv0(x.double().permute(0, 2, 1))
            a = a + rw * torch.relu(blk_conv(a))
            a = a + rw * fc3(torch.relu(fc0(a)))
            return a.permute(0, 2, 1)
    tds.to(dev())
    T = 2400                                          # 1190 output steps: the fp16x3 path (M > 512)
    base = torch.randn(1, T, 80)
    before = ops.range_fallbacks
    y = tds.forward_time_major(base.to(dev()))
    assert ops.range_fallbacks == before              # O(1) activations: the fast form, no fallback
    want = ref(base)
    assert float((y.cpu().double() - want).abs().max()) < 1e-3
    big = base * 3.0e5                                # activations ~1e6 after the first conv: far outside the fp16 range
    y = tds.forward_time_major(big.to(dev()))
    assert ops.range_fallbacks == before + 1          # detected and re-run
    want = ref(big)
    rel = float((y.cpu().double() - want).abs().max() / want.abs().max())
    assert rel < 2e-6, rel                            # fp32 accuracy at the data's own scale, not a clamped fp16 result
    assert float(want.abs().max()) > 65504.0
    # a weight beyond the fp16 range keeps that layer off the fp16x3 form at pack time
    with torch.no_grad():
        tds.blocks[0][1][0].fc[0].weight[0, 0, 0] = 1.0e6
    tds._descriptor()
    assert tds._packs[0]["blocks"][0]["fc0_split"] is None


def test_tds_dense_pair_random_row_counts():
    """The TDS block's dense pair (relu layer -> split-residual layer, split form in and out, under the range guard) at row
    counts that walk every branch of the dispatcher -- 64 x 80 tiles, K-sliced 128 x 160 tiles, 128 x 96 tiles, the 256 x 160
    kernel with and without its K-sliced tail, a 256 x 160 round + a short-input launch for the remaining rows -- against
    float64, with guard rows behind both outputs and a bitwise repeat."""
    from tal_asrd_amd import ops, _native as N_
    lib = N_.lib()
    rng = np.random.default_rng(11)
    rows = {800: [129, 130, 1500, 3200, 3300, 13056, 13057, 13056 + 129, 15001, 17200, 26200],
            1120: [333, 1170, 1200, 4600, 9216 + 200, 9216 + 4096, 9216 + 4097],
            1440: [376, 1819, 1825, 3751, 4267, 4300, 7168 + 64, 7168 + 333, 7501, 12000]}
    for C, ms in rows.items():
        g = torch.Generator().manual_seed(C)
        w0 = (torch.randn(C, C, generator=g) / C ** 0.5).to(dev()); b0 = torch.randn(C, generator=g).to(dev())
        w1 = (torch.randn(C, C, generator=g) / C ** 0.5).to(dev()); b1 = torch.randn(C, generator=g).to(dev())
        w0s, w1s = ops.split_f16x3(w0), ops.split_f16x3(w1)
        w0d, w1d, b0d, b1d = w0.double(), w1.double(), b0.double(), b1.double()
        for M in ms:
            x = torch.randn(M, C, generator=g).to(dev())
            xs = ops.split_f16x3(x)
            nws = lib.tal_linear_workspace_bytes(M, C, C)
            ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=dev())
            flag = torch.zeros(16, dtype=torch.int32, device=dev())
            guard = 2

            def pair():
                hs = torch.full(((M + guard) * C * 4,), 0x5A, dtype=torch.uint8, device=dev())
                ys = torch.full(((M + guard) * C * 4,), 0x5A, dtype=torch.uint8, device=dev())
                N_.check(lib.tal_linear_f16x3_guarded_fwd(N_.ptr(xs), N_.ptr(w0s), N_.ptr(b0), None, 0, 0.0, 1, M, C, C, N_.ptr(hs), 1,
                                                          N_.ptr(flag), N_.ptr(ws), nws, N_.stream_handle()), "relu layer")
                N_.check(lib.tal_linear_f16x3_guarded_fwd(N_.ptr(hs), N_.ptr(w1s), N_.ptr(b1), N_.ptr(xs), 1, 0.3, 2, M, C, C, N_.ptr(ys), 1,
                                                          N_.ptr(flag), N_.ptr(ws), nws, N_.stream_handle()), "residual layer")
                torch.cuda.synchronize()
                return hs, ys

            def decode(buf):
                h = buf[:M * C * 4].view(torch.float16).reshape(M, C // 32, 64).float()
                return (h[:, :, :32] + h[:, :, 32:] / 2048.0).reshape(M, C).double()
            hs, ys = pair()
            hs2, ys2 = pair()
            assert torch.equal(hs, hs2) and torch.equal(ys, ys2), (C, M)
            assert bool((hs[M * C * 4:] == 0x5A).all()) and bool((ys[M * C * 4:] == 0x5A).all()), (C, M)
            xd = decode(xs.view(torch.uint8).reshape(-1))
            hd = decode(hs)
            tol = 2e-5 * max(1.0, C ** 0.5 / 8)
            assert float((hd - torch.relu(xd @ w0d.t() + b0d)).abs().max()) < tol, (C, M)
            assert float((decode(ys) - (xd + 0.3 * (hd @ w1d.t() + b1d))).abs().max()) < tol, (C, M)
            assert int(flag[0]) == 0
