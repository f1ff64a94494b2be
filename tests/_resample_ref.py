"""Float64 yardstick of the resampler: torchaudio 0.4.0's kaldi.resample_waveform restated as mathematics (the package itself is
not available, so parity with it is unpinned; DESIGN.md says so).

For integer rates orig -> new and width = lowpass_filter_width (6):
    g = gcd, iu = orig / g input samples and ou = new / g output phases per unit
    fc = 0.99 * 0.5 * min(orig, new), ww = width / (2 fc)
    phase p: t_p = p / new, first[p] = ceil((t_p - ww) orig), last[p] = floor((t_p + ww) orig), taps = max_p(last - first + 1)
    w[p][j] at dt = (first[p] + j) / orig - t_p: 0 where |dt| >= ww, else
             0.5 (1 + cos(2 pi fc / width dt)) * (sin(2 pi fc dt) / (pi dt), or 2 fc at dt = 0) / orig
    y[q ou + p] = sum_j w[p][j] x[q iu + first[p] + j], x = 0 outside [0, L)
    n_out(L): tick = lcm, last = (L tick / orig) // (tick / new), one less when that division is exact, n_out = last + 1 (0 for L = 0)
"""
import functools
import math

import numpy as np

WIDTH = 6


@functools.lru_cache(maxsize=None)
def plan_f64(orig, new, width=WIDTH):
    """-> (iu, ou, taps, first int64 [ou], w float64 [ou, taps])"""
    g = math.gcd(orig, new)
    iu, ou = orig // g, new // g
    fc = 0.99 * 0.5 * min(orig, new)
    ww = width / (2.0 * fc)
    p = np.arange(ou, dtype=np.float64)
    tp = p / float(new)
    first = np.ceil((tp - ww) * float(orig)).astype(np.int64)
    last = np.floor((tp + ww) * float(orig)).astype(np.int64)
    taps = int((last - first + 1).max())
    j = np.arange(taps, dtype=np.int64)
    dt = (first[:, None] + j[None, :]).astype(np.float64) / float(orig) - tp[:, None]
    win = 0.5 * (1.0 + np.cos(2.0 * np.pi * fc / width * dt))
    safe = np.where(dt == 0.0, 1.0, dt)
    sinc = np.where(dt == 0.0, 2.0 * fc, np.sin(2.0 * np.pi * fc * safe) / (np.pi * safe))
    w = np.where(np.abs(dt) < ww, win * sinc / float(orig), 0.0)
    first.setflags(write=False)
    w.setflags(write=False)
    return iu, ou, taps, first, w


def num_samples(L, orig, new):
    if L <= 0:
        return 0
    tick = orig * new // math.gcd(orig, new)
    ticks_in, per_out = L * (tick // orig), tick // new
    last = ticks_in // per_out
    if last * per_out == ticks_in:
        last -= 1
    return last + 1


def _one(x, orig, new, n_keep):
    """x float64 [L] -> y float64 [n_keep] (the first n_keep outputs of the definition; n_keep <= n_out(L))"""
    iu, ou, taps, first, w = plan_f64(orig, new)
    L = x.shape[0]
    y = np.zeros(n_keep, dtype=np.float64)
    if n_keep == 0:
        return y
    nq = -(-n_keep // ou)
    lo = int(-first.min())
    hi = int((nq - 1) * iu + first.max() + taps)
    xp = np.zeros(lo + max(hi, L), dtype=np.float64)
    xp[lo:lo + L] = x
    q, p = np.divmod(np.arange(n_keep, dtype=np.int64), ou)
    base = q * iu + first[p] + lo
    for j in range(taps):                     # ascending j, every output at once
        y += w[p, j] * xp[base + j]
    return y


def resample_f64(x, orig, new, lengths=None):
    """x [..., L] (any real dtype; int16 is scaled by 2^-15) -> float64 [..., n_out(L)]; with lengths (per row), input at or
    beyond lengths[b] reads as zero and output at or beyond n_out(lengths[b]) is zero (resample, then right-pad)."""
    x = np.asarray(x)
    scale = 2.0 ** -15 if x.dtype == np.int16 else 1.0
    xf = x.astype(np.float64) * scale
    L = xf.shape[-1]
    rows = xf.reshape(-1, L)
    n = num_samples(L, orig, new)
    out = np.zeros((rows.shape[0], n), dtype=np.float64)
    for b in range(rows.shape[0]):
        lb = L if lengths is None else max(0, min(int(lengths[b]), L))
        nb = num_samples(lb, orig, new)
        out[b, :nb] = _one(rows[b, :lb], orig, new, nb)
    return out.reshape(x.shape[:-1] + (n,))


def window_f64(x_slice, slice_start, L, orig, new, m0, count):
    """Outputs m0 .. m0 + count - 1 of an item of L samples of which x_slice = x[slice_start : slice_start + len] is at hand (the
    slice must cover every sample those outputs read inside [0, L)): for spot checks of inputs too long to resample whole."""
    iu, ou, taps, first, w = plan_f64(orig, new)
    xs = np.asarray(x_slice)
    scale = 2.0 ** -15 if xs.dtype == np.int16 else 1.0
    xs = xs.astype(np.float64) * scale
    y = np.zeros(count, dtype=np.float64)
    for i in range(count):
        m = m0 + i
        q, p = divmod(m, ou)
        s = q * iu + int(first[p])
        acc = 0.0
        for j in range(taps):
            idx = s + j
            if 0 <= idx < L and w[p, j] != 0.0:
                k = idx - slice_start
                assert 0 <= k < xs.shape[0], "window_f64: the slice does not cover sample %d" % idx
                acc += w[p, j] * xs[k]
        y[i] = acc
    return y


def err_bound(x, orig, new):
    """A-priori bound of an fp32 evaluation against the float64 one: the weights are rounded to fp32 (2^-24 relative each), the
    products and sums of the `taps`-long FMA chain round once per term (2^-24 of the running magnitude, itself at most
    sum_j |w| max|x|), and one spare unit: (taps + 2) 2^-24 max_p sum_j |w[p][j]| max|x|."""
    _, _, taps, _, w = plan_f64(orig, new)
    x = np.asarray(x)
    scale = 2.0 ** -15 if x.dtype == np.int16 else 1.0
    amax = float(np.abs(x.astype(np.float64)).max()) * scale if x.size else 0.0
    return (taps + 2) * 2.0 ** -24 * float(np.abs(w).sum(axis=1).max()) * amax


def resample_torch(x, orig, new):
    """The reference's own method on a torch tensor x [B, L] (fp32, any device): one strided conv1d per output phase over the
    zero-padded waveform, phases interleaved.  The timing baseline and a second opinion; weights are the fp32-rounded table.
    The convolutions run on PyTorch's native path (im2col + GEMM), not through the vendor convolution library, whose per-shape
    kernel search would dominate a test over a hundred distinct shapes."""
    import torch
    import torch.nn.functional as F
    iu, ou, taps, first, w = plan_f64(orig, new)
    B, L = x.shape
    n = num_samples(L, orig, new)
    nq = -(-n // ou)
    lo = int(-first.min())
    hi = int((nq - 1) * iu + first.max() + taps)
    xp = F.pad(x.unsqueeze(1), (lo, max(hi - L, 0)))
    wt = torch.from_numpy(w.astype(np.float32)).to(x.device)
    was = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        cols = []
        for p in range(min(ou, n)):
            start = lo + int(first[p])
            seg = xp[:, :, start:start + (nq - 1) * iu + taps]
            cols.append(F.conv1d(seg, wt[p].view(1, 1, taps), stride=iu)[:, 0, :nq])
    finally:
        torch.backends.cudnn.enabled = was
    return torch.stack(cols, dim=2).reshape(B, -1)[:, :n]
