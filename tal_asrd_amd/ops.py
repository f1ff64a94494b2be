"""Tensor-level wrappers over the C-ABI (include/tal_asrd.h).  torch is used only
for device memory and the current HIP stream; every op below is a hand-written
HIP kernel and raises if the native library or a GPU is missing.
"""
import ctypes as C

import torch

from . import _native as N


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _f32c(t, what):
    N.require_cuda(t, what)
    if t.dtype != torch.float32:
        raise N.NativeError("%s: expected float32, got %s (only the waveform may be half precision, as the "
                            "reference's call sites hand it over; everything behind the front-end is fp32)" % (what, t.dtype))
    return t.contiguous()


# ------------------------------------------------------------------ log-mel
NFFT_MIN, NFFT_MAX, NMELS_MAX = 32, 2048, 256     # limits of the general front-end (csrc/logmel_general.hip)


class LogmelGeneralPlan:
    """Device plan of the general front-end (tal_logmel_general_*) with the shape it was built for, kept on the host so that a
    call never reads device memory to size its output."""

    def __init__(self, buf, n_fft, hop, n_mels):
        self.buf, self.n_fft, self.hop, self.n_mels = buf, n_fft, hop, n_mels

    @property
    def device(self):
        return self.buf.device


def logmel_shape_error(n_fft, hop, n_mels):
    """-> None if the general front-end takes the shape, else a message naming the violated limit."""
    if not NFFT_MIN <= n_fft <= NFFT_MAX:
        return "n_fft=%d outside %d..%d" % (n_fft, NFFT_MIN, NFFT_MAX)
    if not 1 <= hop <= n_fft:
        return "hop=%d outside 1..n_fft (%d)" % (hop, n_fft)
    if not 1 <= n_mels <= NMELS_MAX:
        return "n_mels=%d outside 1..%d" % (n_mels, NMELS_MAX)
    return None


def logmel_plan(window, fb, hop=160):
    """Device plan for log-mel: window [n_fft], fb [n_fft//2 + 1, n_mels].  The default shape (400, hop 160, 80 mels) gets the
    plan of tal_logmel_fwd (a uint8 tensor) unless the option `logmel_general` is set; any other shape a LogmelGeneralPlan."""
    lib = N.lib()
    window = _f32c(window, "logmel_plan(window)")
    fb = _f32c(fb, "logmel_plan(fb)")
    if window.dim() != 1 or fb.dim() != 2 or fb.shape[0] != window.shape[0] // 2 + 1:
        raise N.NativeError("logmel_plan: window/fb must be [n_fft] and [n_fft//2 + 1, n_mels], got %s %s"
                            % (tuple(window.shape), tuple(fb.shape)))
    n_fft, n_mels = int(window.shape[0]), int(fb.shape[1])
    if (n_fft, hop, n_mels) != (400, 160, 80) or N.get_option("logmel_general"):
        err = logmel_shape_error(n_fft, hop, n_mels)
        if err:
            raise N.NativeError("logmel_plan: " + err)
        buf = torch.empty(lib.tal_logmel_general_plan_bytes(n_fft, n_mels), dtype=torch.uint8, device=window.device)
        N.check(lib.tal_logmel_general_plan_init(N.ptr(window), n_fft, hop, N.ptr(fb), n_mels, N.ptr(buf), N.stream_handle()),
                "tal_logmel_general_plan_init")
        return LogmelGeneralPlan(buf, n_fft, hop, n_mels)
    plan = torch.empty(lib.tal_logmel_plan_bytes(), dtype=torch.uint8, device=window.device)
    N.check(lib.tal_logmel_plan_init(N.ptr(window), N.ptr(fb), N.ptr(plan), N.stream_handle()),
            "tal_logmel_plan_init")
    return plan


def _audio(t, what):
    """The waveform is the one tensor the reference's callers hand over in half precision (`audio_x.half()`,
    tal/asr/system.py:92,285; `x_wav.cuda().half()`, tal/baseline/reconcile.py:78): fp16 and fp32 are both taken as they
    are (the kernel widens fp16 samples while it stages them); anything else raises."""
    N.require_cuda(t, what)
    if t.dtype not in (torch.float32, torch.float16):
        raise N.NativeError("%s: the waveform must be float32 or float16, got %s%s" % (what, t.dtype, (
            " (16-bit PCM goes through tal_asrd_amd.Resample(orig_freq, new_freq), or the sample_rate= argument of the models' "
            "entry points, which scale it by 2^-15 on the device)") if t.dtype == torch.int16 else ""))
    return t.contiguous()


def logmel(plan, audio, eps=1e-6, subtract_mean=True, return_stats=False):
    """audio [B, L] fp32 or fp16 -> [B, T, n_mels] fp32 (LogMelSpec.forward, tal/asr/models.py:35-53); T = 1 + L // hop as
    torch.stft counts for even n_fft (the default plan: [B, T, 80]), 1 + (L - 1) // hop for odd n_fft."""
    lib = N.lib()
    audio = _audio(audio, "logmel")
    if audio.dim() != 2:
        raise N.NativeError("logmel: audio must be [batch, samples]")
    B, L = audio.shape
    if isinstance(plan, LogmelGeneralPlan):
        T = lib.tal_logmel_frames(L - plan.n_fft % 2, plan.hop)        # (torch.stft's count: one less for odd n_fft when hop | L)
        out = torch.empty(B, T, plan.n_mels, dtype=torch.float32, device=audio.device)
        mean = torch.empty(1, dtype=torch.float32, device=audio.device)
        stats = torch.empty(2, dtype=torch.float64, device=audio.device)
        nws = lib.tal_logmel_general_workspace_bytes(plan.n_fft, plan.hop, B, L)
        ws = _ws(nws, audio.device)
        N.check(lib.tal_logmel_general_fwd(N.ptr(plan.buf), plan.n_fft, plan.hop, plan.n_mels, N.ptr(audio),
                                           1 if audio.dtype == torch.float16 else 0, B, L, eps, 1 if subtract_mean else 0,
                                           N.ptr(out), N.ptr(mean), N.ptr(stats), N.ptr(ws), nws, N.stream_handle()),
                "tal_logmel_general_fwd")
        return (out, mean, stats) if return_stats else out
    T = lib.tal_logmel_num_frames(L)
    out = torch.empty(B, T, 80, dtype=torch.float32, device=audio.device)
    mean = torch.empty(1, dtype=torch.float32, device=audio.device)
    stats = torch.empty(2, dtype=torch.float64, device=audio.device)
    nws = lib.tal_logmel_workspace_bytes(B, L)
    ws = _ws(nws, audio.device)
    fwd = lib.tal_logmel_f16_fwd if audio.dtype == torch.float16 else lib.tal_logmel_fwd
    N.check(fwd(N.ptr(plan), N.ptr(audio), B, L, eps, 1 if subtract_mean else 0, N.ptr(out),
                N.ptr(mean), N.ptr(stats), N.ptr(ws), nws, N.stream_handle()), "tal_logmel_fwd")
    return (out, mean, stats) if return_stats else out


def subtract_scalar_(x, mean):
    lib = N.lib()
    N.check(lib.tal_subtract_scalar(N.ptr(x), x.numel(), N.ptr(mean), N.stream_handle()), "tal_subtract_scalar")
    return x


# ------------------------------------------------------------------ resampling
RESAMPLE_WIDTH = 6        # torchaudio's lowpass_filter_width default, the only one the reference uses
_RESAMPLE_DTYPES = {torch.float32: 0, torch.float16: 1, torch.int16: 2}     # TAL_RESAMPLE_F32 / _F16 / _I16


class ResamplePlan:
    """Device table of one rate pair (tal_resample_plan_init) with the pair it was built for."""

    def __init__(self, buf, orig, new, width):
        self.buf, self.orig, self.new, self.width = buf, orig, new, width

    @property
    def device(self):
        return self.buf.device


def _rate(v, what):
    if isinstance(v, bool) or int(v) != v:
        raise N.NativeError("%s: sample rates are integers (Hz), got %r" % (what, v))
    return int(v)


def resample_plan_bytes(orig, new, width=RESAMPLE_WIDTH):
    """Bytes of the pair's device plan; raises with the violated limit outside the limits (host arithmetic, no GPU)."""
    lib = N.lib()
    orig, new = _rate(orig, "resample_plan"), _rate(new, "resample_plan")
    if max(abs(orig), abs(new)) >= 2 ** 31:
        raise N.NativeError("resample_plan(%d -> %d): sample rates must be 1..1048576 Hz" % (orig, new))
    nbytes = lib.tal_resample_plan_bytes(orig, new, width)
    if nbytes == 0:
        # the host builder's message names the limit that is violated
        N.check(lib.tal_resample_plan_build_host(orig, new, width, None, None, None), "resample_plan(%d -> %d)" % (orig, new))
        raise N.NativeError("resample_plan(%d -> %d): outside the plan limits" % (orig, new))
    return nbytes


def resample_plan(orig, new, device, width=RESAMPLE_WIDTH):
    lib = N.lib()
    nbytes = resample_plan_bytes(orig, new, width)
    device = torch.device(device)
    if device.type != "cuda":
        raise N.NativeError("resample_plan: the hot path only runs on the GPU (HIP kernels); got device %s and there is deliberately "
                            "no CPU fallback" % device)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        N.check(lib.tal_resample_plan_init(N.ptr(buf), int(orig), int(new), width, N.stream_handle()), "tal_resample_plan_init")
    return ResamplePlan(buf, int(orig), int(new), width)


def resample_num_samples(n_in, orig, new):
    """Samples out for n_in samples in (an int, or an integer tensor mapped element by element on the host, as audio_lens)."""
    lib = N.lib()
    orig, new = _rate(orig, "resample_num_samples"), _rate(new, "resample_num_samples")
    if isinstance(n_in, torch.Tensor):
        flat = [lib.tal_resample_num_samples(int(v), orig, new) for v in n_in.detach().cpu().reshape(-1).tolist()]
        return torch.tensor(flat, dtype=torch.int64).reshape(n_in.shape)
    return lib.tal_resample_num_samples(int(n_in), orig, new)


def resample(plan, x, lengths=None):
    """x [..., L] fp32 / fp16 / int16 (16-bit PCM, scaled by 2^-15) -> fp32 [..., n_out(L)] at plan.new Hz (tal_resample_fwd).
    lengths (one per row of x, in input samples): input at or beyond it reads as zero, output at or beyond n_out(length) is zero."""
    lib = N.lib()
    N.require_cuda(x, "resample")
    if x.dtype not in _RESAMPLE_DTYPES:
        raise N.NativeError("resample: the waveform must be float32, float16 or int16, got %s" % x.dtype)
    if x.dim() < 1:
        raise N.NativeError("resample: the waveform must be [..., samples]")
    if x.device != plan.device:
        raise N.NativeError("resample: the plan lives on %s, the waveform on %s" % (plan.device, x.device))
    L = x.shape[-1]
    lead = tuple(x.shape[:-1])
    n = lib.tal_resample_num_samples(L, plan.orig, plan.new)
    if not (x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= L) and not x.is_contiguous():
        x = x.contiguous()
    B = 1
    for d in lead:
        B *= d
    pitch = x.stride(0) if x.dim() == 2 and B > 1 else L      # (rows of a 2-D view may be further apart than L)
    y = torch.empty(lead + (n,), dtype=torch.float32, device=x.device)
    if lengths is not None:
        lengths = torch.as_tensor(lengths).to(device=x.device, dtype=torch.int64).contiguous()
        if lengths.numel() != B:
            raise N.NativeError("resample: %d lengths for %d rows" % (lengths.numel(), B))
    if B == 0 or n == 0:
        return y
    N.check(lib.tal_resample_fwd(N.ptr(plan.buf), plan.orig, plan.new, plan.width, N.ptr(x), _RESAMPLE_DTYPES[x.dtype], B, L, pitch,
                                 N.ptr(lengths), N.ptr(y), n, N.stream_handle()), "tal_resample_fwd")
    return y


# ------------------------------------------------------------------ dense
def linear(x, weight, bias=None, mode=0, res=None, alpha=0.0, out=None):
    """y = epilogue(x . W^T + b) over the last dim; weight [N, K] (nn.Linear / 1x1 Conv1d layout)."""
    lib = N.lib()
    x = _f32c(x, "linear")
    w2 = weight.reshape(weight.shape[0], -1)
    w2 = _f32c(w2, "linear(weight)")
    K = x.shape[-1]
    Nout = w2.shape[0]
    if w2.shape[1] != K:
        raise N.NativeError("linear: x[..., %d] vs weight %s" % (K, tuple(weight.shape)))
    M = x.numel() // K
    y = out if out is not None else torch.empty(*x.shape[:-1], Nout, dtype=torch.float32, device=x.device)
    if res is not None:
        res = _f32c(res, "linear(res)")
    if bias is not None:
        bias = _f32c(bias, "linear(bias)")
    nws = lib.tal_linear_workspace_bytes(M, Nout, K)
    if nws:
        ws = _ws(nws, x.device)    # (torch's caching allocator hands the same block back call after call)
        N.check(lib.tal_linear_ws_fwd(N.ptr(x), N.ptr(w2), N.ptr(bias), N.ptr(res), float(alpha), int(mode), M, Nout, K,
                                      N.ptr(y), N.ptr(ws), nws, N.stream_handle()), "tal_linear_ws_fwd")
    else:
        N.check(lib.tal_linear_fwd(N.ptr(x), N.ptr(w2), N.ptr(bias), N.ptr(res), float(alpha), int(mode), M, Nout, K,
                                   N.ptr(y), N.stream_handle()), "tal_linear_fwd")
    return y


def split_f16x3(x2d):
    """fp32 [rows, K] (K % 32 == 0) -> the hi / lo fp16 split the fp16x3 dense layers consume (same number of bytes,
    returned as an opaque uint8 tensor)."""
    lib = N.lib()
    x2d = _f32c(x2d, "split_f16x3")
    rows, K = x2d.shape
    out = torch.empty(rows * K * 4, dtype=torch.uint8, device=x2d.device)
    N.check(lib.tal_split_f16x3_fwd(N.ptr(x2d), N.ptr(out), rows, K, N.stream_handle()), "tal_split_f16x3_fwd")
    return out


# ------------------------------------------------------------------ grouped conv
def pack_gconv_weight(weight, groups):
    """reference Conv1d weight [C_out, C_in/G, k] -> packed [G][C_in/G][k][C_out/G] (1 <= k <= TAL_GCONV_MAX_K)."""
    lib = N.lib()
    w = _f32c(weight, "pack_gconv_weight")
    c_out, cig, ks = w.shape
    packed = torch.empty(w.numel(), dtype=torch.float32, device=w.device)
    N.check(lib.tal_pack_gconv_weight(N.ptr(w), N.ptr(packed), c_out, cig, ks, groups, N.stream_handle()),
            "tal_pack_gconv_weight")
    return packed


def gconv_s2(x, w_packed, bias, c_out, groups, ksize=21):
    """x [B, T, C_in] -> [B, (T-k)//2+1, C_out] (tal/asr/models.py:363-364); k != 21 runs the any-k kernel (gconv_s2_k)."""
    if ksize != 21:
        return gconv_s2_k(x, w_packed, bias, c_out, groups, ksize)
    lib = N.lib()
    x = _f32c(x, "gconv_s2")
    B, T, c_in = x.shape
    y = torch.empty(B, (T - 21) // 2 + 1, c_out, dtype=torch.float32, device=x.device)
    N.check(lib.tal_gconv_s2_fwd(N.ptr(x), N.ptr(w_packed), N.ptr(bias), B, T, c_in, c_out, groups, N.ptr(y),
                                 N.stream_handle()), "tal_gconv_s2_fwd")
    return y


def gconv_res(x, w_packed, bias, alpha, groups, ksize=21):
    """x + alpha * relu(gconv_k(x)) on [B, T, C] (tal/asr/models.py:304-308,329); k != 21 runs the any-k kernel (gconv_res_k)."""
    if ksize != 21:
        return gconv_res_k(x, w_packed, bias, alpha, groups, ksize)
    lib = N.lib()
    x = _f32c(x, "gconv_res")
    B, T, c = x.shape
    y = torch.empty_like(x)
    N.check(lib.tal_gconv_res_fwd(N.ptr(x), N.ptr(w_packed), N.ptr(bias), float(alpha), B, T, c, groups, N.ptr(y),
                                  N.stream_handle()), "tal_gconv_res_fwd")
    return y


def gconv_s2_k(x, w_packed, bias, c_out, groups, ksize):
    """The stride-2 resize conv at any kernel size 1..TAL_GCONV_MAX_K (tal_gconv_s2_k_fwd, exact fp32; bit-identical to
    gconv_s2 at k = 21): x [B, T, C_in] -> [B, (T-k)//2+1, C_out]."""
    lib = N.lib()
    x = _f32c(x, "gconv_s2_k")
    B, T, c_in = x.shape
    if T < ksize:
        raise N.NativeError("gconv_s2_k: %d frames are too few for kernel size %d" % (T, ksize))
    y = torch.empty(B, (T - ksize) // 2 + 1, c_out, dtype=torch.float32, device=x.device)
    N.check(lib.tal_gconv_s2_k_fwd(N.ptr(x), N.ptr(w_packed), N.ptr(bias), B, T, c_in, c_out, groups, int(ksize), N.ptr(y),
                                   N.stream_handle()), "tal_gconv_s2_k_fwd")
    return y


def gconv_res_k(x, w_packed, bias, alpha, groups, ksize):
    """x + alpha * relu(gconv_k(x)) at any odd kernel size 1..TAL_GCONV_MAX_K (tal_gconv_res_k_fwd, exact fp32; bit-identical to
    gconv_res at k = 21)."""
    lib = N.lib()
    x = _f32c(x, "gconv_res_k")
    B, T, c = x.shape
    y = torch.empty_like(x)
    N.check(lib.tal_gconv_res_k_fwd(N.ptr(x), N.ptr(w_packed), N.ptr(bias), float(alpha), B, T, c, groups, int(ksize), N.ptr(y),
                                    N.stream_handle()), "tal_gconv_res_k_fwd")
    return y


def pack_gconv_f16x3_weight(weight, groups, stride=1):
    """reference Conv1d weight [C_out, C_in/G, 21] -> fp16x3 MFMA operand fragments (opaque uint8 tensor), or None when
    the shape has no matrix-core kernel (tal_gconv_f16x3_weight_bytes == 0)."""
    lib = N.lib()
    w = _f32c(weight, "pack_gconv_f16x3_weight")
    c_out, cig, ks = w.shape
    c_in = cig * groups
    nbytes = lib.tal_gconv_f16x3_weight_bytes(c_in, c_out, groups, stride) if ks == 21 else 0
    if nbytes == 0:
        return None
    frag = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    N.check(lib.tal_pack_gconv_f16x3_weight(N.ptr(w), N.ptr(frag), c_in, c_out, groups, stride, N.stream_handle()),
            "tal_pack_gconv_f16x3_weight")
    return frag


def gconv_s2_f16x3(x, w_frag, bias, c_out, groups):
    """x [B, T, C_in] -> [B, (T-21)//2+1, C_out] (tal/asr/models.py:363-364) on the matrix cores (fp16x3 form)."""
    lib = N.lib()
    x = _f32c(x, "gconv_s2_f16x3")
    B, T, c_in = x.shape
    y = torch.empty(B, (T - 21) // 2 + 1, c_out, dtype=torch.float32, device=x.device)
    N.check(lib.tal_gconv_s2_f16x3_fwd(N.ptr(x), N.ptr(w_frag), N.ptr(bias), B, T, c_in, c_out, groups, N.ptr(y),
                                       N.stream_handle()), "tal_gconv_s2_f16x3_fwd")
    return y


def gconv_res_f16x3(x, w_frag, bias, alpha, groups, want_split=False):
    """x + alpha * relu(gconv21(x)) on [B, T, C] on the matrix cores (fp16x3 form); with want_split also returns the
    result as the hi / lo split the fp16x3 dense layers consume (split_f16x3's format)."""
    lib = N.lib()
    x = _f32c(x, "gconv_res_f16x3")
    B, T, c = x.shape
    y = torch.empty_like(x)
    ys = torch.empty(B * T * c * 4, dtype=torch.uint8, device=x.device) if want_split else None
    N.check(lib.tal_gconv_res_f16x3_fwd(N.ptr(x), N.ptr(w_frag), N.ptr(bias), float(alpha), B, T, c, groups, N.ptr(y),
                                        N.ptr(ys) if want_split else None, N.stream_handle()), "tal_gconv_res_f16x3_fwd")
    return (y, ys) if want_split else y


def gconv_res_split(x_split, shape, w_frag, bias, alpha, groups):
    """TDSBlock conv on activations in the hi / lo split form: x_split (opaque uint8 tensor, split_f16x3's format) of
    logical shape [B, T, C] -> the split form of x + alpha * relu(gconv21(x))."""
    lib = N.lib()
    B, T, c = shape
    ys = torch.empty(B * T * c * 4, dtype=torch.uint8, device=x_split.device)
    N.check(lib.tal_gconv_res_split_fwd(N.ptr(x_split), N.ptr(w_frag), N.ptr(bias), float(alpha), B, T, c, groups, N.ptr(ys),
                                        N.stream_handle()), "tal_gconv_res_split_fwd")
    return ys


def gconv_s2_split(x, shape, x_is_split, w_frag, bias, c_out, groups):
    """Stride-2 resize conv writing the split form of its output; x is fp32 [B, T, C_in] or the split form of it."""
    lib = N.lib()
    B, T, c_in = shape
    t_out = (T - 21) // 2 + 1
    ys = torch.empty(B * t_out * c_out * 4, dtype=torch.uint8, device=x.device)
    N.check(lib.tal_gconv_s2_split_fwd(N.ptr(x), 1 if x_is_split else 0, N.ptr(w_frag), N.ptr(bias), B, T, c_in, c_out, groups,
                                       N.ptr(ys), N.stream_handle()), "tal_gconv_s2_split_fwd")
    return ys


# ------------------------------------------------------------------ TDS driver
range_fallbacks = 0      # calls that were re-run on the exact fp32 kernels because an activation left the fp16 range


class RangeCheck:
    """Pending fp16-range check of one tal_tds_fwd call: `flagged()` reads the call's status word (a 4-byte device-to-host
    copy, i.e. a wait for the stream), `rerun_exact()` repeats the call on the exact fp32-input kernels into the same
    output tensor.  Deferring the read lets the caller enqueue the kernels that consume the encoder output first."""

    def __init__(self, desc, x, y, ws, nws, off, x_mean=None, y_split=False):
        self.desc, self.x, self.y, self.ws, self.nws, self.off, self.x_mean = desc, x, y, ws, nws, off, x_mean
        self.y_split = y_split          # y holds the hi / lo split form (tds_forward(out_split=True)); an exact re-run writes fp32

    def flagged(self):
        """One 8-byte read of the call's status block: word 0 = an activation left the fp16 range; word 1 = the form the call
        wrote y in, which must be the form `y_split` promised the consumer (tal_tds_out_split is a prediction: another thread's
        tal_set_option between the query and the call, or a misaligned x, changes what the call does -- never silently)."""
        if self.desc.flags & N.TAL_TDS_EXACT_F32 and not self.y_split:
            return False
        flag, form = self.ws[self.off:self.off + 8].view(torch.int32).tolist()
        if bool(form) != bool(self.y_split):
            raise N.NativeError("tal_tds_fwd wrote its output in the %s form but its consumer was enqueued for the %s form "
                                "(a kernel-selection option changed between tal_tds_out_split and the call?)"
                                % ("split" if form else "fp32", "split" if self.y_split else "fp32"))
        return flag != 0 and not (self.desc.flags & N.TAL_TDS_EXACT_F32)

    def rerun_exact(self):
        global range_fallbacks
        range_fallbacks += 1
        lib = N.lib()
        B, T, _ = self.x.shape
        exact = N.TdsDesc.from_buffer_copy(self.desc)       # (a copy: the cached descriptor may be in use by another thread's call)
        exact.flags |= N.TAL_TDS_EXACT_F32
        N.check(_tds_call(lib, exact, self.x, self.x_mean, B, T, self.y, self.ws, self.nws), "tal_tds_fwd (exact fp32 re-run)")
        self.y_split = False
        return self.y


def _tds_call(lib, desc, x, x_mean, B, T, y, ws, nws):
    if x_mean is None:
        return lib.tal_tds_fwd(C.byref(desc), N.ptr(x), B, T, N.ptr(y), N.ptr(ws), nws, N.stream_handle())
    return lib.tal_tds_premean_fwd(C.byref(desc), N.ptr(x), N.ptr(x_mean), B, T, N.ptr(y), N.ptr(ws), nws, N.stream_handle())


def tds_premean_ok(desc, x):
    """May `x` be handed to tds_forward as a log-mel BEFORE its mean subtraction (x_mean=...)?  (tal_tds_premean_ok)"""
    return bool(N.lib().tal_tds_premean_ok(C.byref(desc), N.ptr(x)))


def tds_forward(desc, x, c_out, check_range=True, defer=False, x_mean=None, out_split=False):
    """x [B, T, C0] -> [B, T', C_last] through tal_tds_fwd (whole encoder, one C call).

    x_mean (device tensor [1]): x is the log-mel before LogMelSpec's global-mean subtraction and x_mean the scalar to subtract
    (logmel(..., subtract_mean=False, return_stats=True)); the subtraction is folded into the first resize conv's bias
    (tal_tds_premean_fwd).  Only where tds_premean_ok(desc, x).

    out_split=True (with defer=True): the caller's consumer takes the hi / lo split form (sd_head(x_split=True)); where the last
    stage runs all-split the output tensor then holds that form -- same shape and bytes, NOT fp32 values -- and the returned
    RangeCheck says so (`.y_split`).

    fp16-range guard: the long-input layers run in the fp16x3 form (fp32 values as two fp16 halves), which needs
    |activation| <= 65504.  The kernels raise a status word when a value was out of range; the call is then repeated
    on the exact fp32-input kernels (one small device-to-host read per call; check_range=False skips it).
    defer=True returns (y, RangeCheck) and leaves the read to the caller (after it has enqueued the consumers of y)."""
    lib = N.lib()
    x = _f32c(x, "tds_forward")
    B, T, _ = x.shape
    t_out = lib.tal_tds_out_len(C.byref(desc), T)
    if t_out <= 0:
        raise N.NativeError("tds_forward: %d frames are too few for the stride-2 k=%d stages" % (T, desc.ksize or 21))
    y = torch.empty(B, t_out, c_out, dtype=torch.float32, device=x.device)
    nws = lib.tal_tds_workspace_bytes(C.byref(desc), B, T)
    ws = _ws(nws, x.device)
    y_split = False
    if out_split:
        if not defer:
            raise N.NativeError("tds_forward: out_split needs defer=True (the caller must look at RangeCheck.y_split)")
        asked = N.TdsDesc.from_buffer_copy(desc)
        asked.flags |= N.TAL_TDS_OUT_SPLIT
        if lib.tal_tds_out_split(C.byref(asked), B, T):
            desc, y_split = asked, True
    N.check(_tds_call(lib, desc, x, x_mean, B, T, y, ws, nws), "tal_tds_fwd")
    chk = RangeCheck(desc, x, y, ws, nws, lib.tal_tds_status_offset(C.byref(desc), B, T), x_mean, y_split)
    if defer:
        return y, chk
    if check_range and chk.flagged():
        chk.rerun_exact()
    return y


def tds_forward_tiled(desc, x, c_out, out_tile, check_range=True):
    """x [1, T, C0] -> [1, T', C_last] through tal_tds_tiled_fwd: tiles of `out_tile` output frames, each with its
    receptive-field halo (include/tal_asrd.h); same range guard as tds_forward."""
    lib = N.lib()
    x = _f32c(x, "tds_forward_tiled")
    if x.dim() != 3 or x.shape[0] != 1:
        raise N.NativeError("tds_forward_tiled: x must be [1, T, C]")
    T = x.shape[1]
    t_out = lib.tal_tds_out_len(C.byref(desc), T)
    if t_out <= 0:
        raise N.NativeError("tds_forward_tiled: %d frames are too few for the stride-2 k=%d stages" % (T, desc.ksize or 21))
    y = torch.empty(1, t_out, c_out, dtype=torch.float32, device=x.device)
    nws = lib.tal_tds_tiled_workspace_bytes(C.byref(desc), T, int(out_tile))
    ws = _ws(nws, x.device)

    def run(d):
        N.check(lib.tal_tds_tiled_fwd(C.byref(d), N.ptr(x), T, N.ptr(y), int(out_tile), N.ptr(ws), nws, N.stream_handle()),
                "tal_tds_tiled_fwd")
    run(desc)
    if check_range and not (desc.flags & N.TAL_TDS_EXACT_F32):
        off = lib.tal_tds_tiled_status_offset(C.byref(desc), T, int(out_tile))
        if int(ws[off:off + 4].view(torch.int32)[0]) != 0:
            global range_fallbacks
            range_fallbacks += 1
            exact = N.TdsDesc.from_buffer_copy(desc)
            exact.flags |= N.TAL_TDS_EXACT_F32
            run(exact)
    return y


# ------------------------------------------------------------------ diarization head
def sd_head(x, w_embed, b_embed, w_logit, b_logit, want_logits=True, want_ids=True, x_split=False, w_embed_split=None):
    """x [..., C] -> (feat [..., E], logits [..., S] | None, ids [...] int32 | None).
    x_split=True: x holds the hi / lo split form (tds_forward(out_split=True) with RangeCheck.y_split) and w_embed_split the
    split of w_embed (split_f16x3): the embedding layer runs in the fp16x3 form (tal_sd_head_split_fwd)."""
    lib = N.lib()
    x = _f32c(x, "sd_head")
    Cc = x.shape[-1]
    M = x.numel() // Cc
    E, S = w_embed.shape[0], w_logit.shape[0]
    dev = x.device
    feat = torch.empty(*x.shape[:-1], E, dtype=torch.float32, device=dev)
    logits = torch.empty(*x.shape[:-1], S, dtype=torch.float32, device=dev) if want_logits else None
    ids = torch.empty(x.shape[:-1], dtype=torch.int32, device=dev) if want_ids else None
    # (features alone take the workspace too: the embedding layer of a medium input is then the K-sliced launch of the ids call, so
    #  spk_topk's features are speaker_ids' features bit for bit)
    nws = lib.tal_sd_head_workspace_bytes(M, S) if not want_logits else 0
    ws = _ws(nws, dev)
    if x_split:
        if w_embed_split is None:
            raise N.NativeError("sd_head: x_split needs w_embed_split (ops.split_f16x3 of the embedding weight)")
        if not nws:
            nws = lib.tal_sd_head_workspace_bytes(M, S)
            ws = _ws(nws, dev)
        N.check(lib.tal_sd_head_split_fwd(N.ptr(x), M, Cc, N.ptr(w_embed_split), N.ptr(b_embed), E,
                                          N.ptr(_f32c(w_logit, "w")), N.ptr(b_logit), S, N.ptr(feat), N.ptr(logits),
                                          N.ptr(ids), N.ptr(ws), nws, N.stream_handle()), "tal_sd_head_split_fwd")
        return feat, logits, ids
    N.check(lib.tal_sd_head_fwd(N.ptr(x), M, Cc, N.ptr(_f32c(w_embed, "w")), N.ptr(b_embed), E,
                                N.ptr(_f32c(w_logit, "w")), N.ptr(b_logit), S, N.ptr(feat), N.ptr(logits),
                                N.ptr(ids), N.ptr(ws), nws, N.stream_handle()), "tal_sd_head_fwd")
    return feat, logits, ids


def argmax_rows(x):
    lib = N.lib()
    x = _f32c(x, "argmax_rows")
    Nn = x.shape[-1]
    M = x.numel() // Nn
    ids = torch.empty(x.shape[:-1], dtype=torch.int32, device=x.device)
    N.check(lib.tal_argmax_rows(N.ptr(x), M, Nn, N.ptr(ids), N.stream_handle()), "tal_argmax_rows")
    return ids


def _check_k(k, n, what):
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= min(N.TAL_TOPK_MAX, n):
        raise N.NativeError("%s: k=%r outside 1..min(%d, %d columns)" % (what, k, N.TAL_TOPK_MAX, n))
    return int(k)


def spk_topk(feat, w_logit, b_logit, k):
    """feat [..., E] -> (ids [..., k] int32, logp [..., k], lse [...]) of the speaker posterior softmax(feat . w_logit^T + b_logit)
    without the logits in memory (tal_spk_topk_fwd): the k largest per row, value descending and index ascending among equal values,
    logp = logit - lse.  b_logit None = zeros; a -inf bias entry masks that speaker."""
    lib = N.lib()
    feat = _f32c(feat, "spk_topk")
    w = _f32c(w_logit, "spk_topk(w_logit)")
    b = None if b_logit is None else _f32c(b_logit, "spk_topk(b_logit)")
    E, S = feat.shape[-1], w.shape[0]
    if w.dim() != 2 or w.shape[1] != E or (b is not None and b.numel() != S):
        raise N.NativeError("spk_topk: feat [..., %d] vs w_logit %s, b_logit %s"
                            % (E, tuple(w.shape), None if b is None else tuple(b.shape)))
    k = _check_k(k, S, "spk_topk")
    M = feat.numel() // E
    lead, dev = tuple(feat.shape[:-1]), feat.device
    ids = torch.empty(lead + (k,), dtype=torch.int32, device=dev)
    logp = torch.empty(lead + (k,), dtype=torch.float32, device=dev)
    lse = torch.empty(lead, dtype=torch.float32, device=dev)
    nws = lib.tal_spk_topk_workspace_bytes(M, S, E, k)
    ws = _ws(nws, dev)
    N.check(lib.tal_spk_topk_fwd(N.ptr(feat), M, E, N.ptr(w), N.ptr(b), S, k, N.ptr(ids), N.ptr(logp), N.ptr(lse), N.ptr(ws), nws,
                                 N.stream_handle()), "tal_spk_topk_fwd")
    return ids, logp, lse


def topk_lse_rows(x, k):
    """x [..., n] -> (ids [..., k] int32, logp [..., k], lse [...]): the same reduction over a materialised matrix (tal_topk_lse_rows)."""
    lib = N.lib()
    x = _f32c(x, "topk_lse_rows")
    Nn = x.shape[-1]
    k = _check_k(k, Nn, "topk_lse_rows")
    M = x.numel() // Nn
    lead = tuple(x.shape[:-1])
    ids = torch.empty(lead + (k,), dtype=torch.int32, device=x.device)
    logp = torch.empty(lead + (k,), dtype=torch.float32, device=x.device)
    lse = torch.empty(lead, dtype=torch.float32, device=x.device)
    N.check(lib.tal_topk_lse_rows(N.ptr(x), M, Nn, k, N.ptr(ids), N.ptr(logp), N.ptr(lse), N.stream_handle()), "tal_topk_lse_rows")
    return ids, logp, lse


def _targets(target, lead, what):
    """int64 targets of the leading shape `lead`, contiguous on the device (any integer dtype is widened)."""
    N.require_cuda(target, what)
    if target.dtype.is_floating_point or target.dtype == torch.bool or tuple(target.shape) != tuple(lead):
        raise N.NativeError("%s: targets must be integers of shape %s, got %s %s" % (what, tuple(lead), target.dtype, tuple(target.shape)))
    return target.to(torch.int64).contiguous()


def xent_rows(feat, w, bias, target, want_lse=False, want_top1=False):
    """feat [..., E], target [...] -> nll [...] (and lse [...], top1 [...] int32 on request) of softmax(feat . w^T + bias) without
    the logits in memory (tal_xent_rows_fwd): nll = lse - logit[target]; a negative target skips the row (nll = 0), a target past the
    head gives +inf; top1 is the arg-max with the first index among equal values.  bias None = zeros; a -inf entry masks a column."""
    lib = N.lib()
    feat = _f32c(feat, "xent_rows")
    w = _f32c(w, "xent_rows(w)")
    b = None if bias is None else _f32c(bias, "xent_rows(bias)")
    E, S = feat.shape[-1], w.shape[0]
    if w.dim() != 2 or w.shape[1] != E or (b is not None and b.numel() != S):
        raise N.NativeError("xent_rows: feat [..., %d] vs w %s, bias %s" % (E, tuple(w.shape), None if b is None else tuple(b.shape)))
    lead, dev = tuple(feat.shape[:-1]), feat.device
    t = _targets(target, lead, "xent_rows(target)")
    M = feat.numel() // E
    nll = torch.empty(lead, dtype=torch.float32, device=dev)
    lse = torch.empty(lead, dtype=torch.float32, device=dev) if want_lse else None
    top1 = torch.empty(lead, dtype=torch.int32, device=dev) if want_top1 else None
    nws = lib.tal_xent_rows_workspace_bytes(M, S, E)
    ws = _ws(nws, dev)
    N.check(lib.tal_xent_rows_fwd(N.ptr(feat), M, E, E, N.ptr(w), N.ptr(b), S, N.ptr(t), N.ptr(nll), N.ptr(lse), N.ptr(top1), N.ptr(ws),
                                  nws, N.stream_handle()), "tal_xent_rows_fwd")
    return (nll,) + ((lse,) if want_lse else ()) + ((top1,) if want_top1 else ()) if want_lse or want_top1 else nll


def xent_lse_rows(x, target, want_lse=False, want_top1=False):
    """x [..., n], target [...] -> nll (lse, top1 on request): the same reduction over a materialised matrix (tal_xent_lse_rows)."""
    lib = N.lib()
    x = _f32c(x, "xent_lse_rows")
    Nn = x.shape[-1]
    lead = tuple(x.shape[:-1])
    t = _targets(target, lead, "xent_lse_rows(target)")
    M = x.numel() // Nn
    nll = torch.empty(lead, dtype=torch.float32, device=x.device)
    lse = torch.empty(lead, dtype=torch.float32, device=x.device) if want_lse else None
    top1 = torch.empty(lead, dtype=torch.int32, device=x.device) if want_top1 else None
    N.check(lib.tal_xent_lse_rows(N.ptr(x), M, Nn, N.ptr(t), N.ptr(nll), N.ptr(lse), N.ptr(top1), N.stream_handle()), "tal_xent_lse_rows")
    return (nll,) + ((lse,) if want_lse else ()) + ((top1,) if want_top1 else ()) if want_lse or want_top1 else nll


def soft_embed(feat, w, bias, values=None, want_lse=False):
    """feat [..., E] -> out [..., D] (and lse [...] on request): softmax(feat . w^T + bias) . values without the logits or the
    probabilities in memory (tal_soft_embed_fwd).  values [n, D]; None: values = w (the soft embedding of a tied head, D = E).
    bias None = zeros; a -inf entry masks a column."""
    lib = N.lib()
    feat = _f32c(feat, "soft_embed")
    w = _f32c(w, "soft_embed(w)")
    b = None if bias is None else _f32c(bias, "soft_embed(bias)")
    v = None if values is None else _f32c(values, "soft_embed(values)")
    E, S = feat.shape[-1], w.shape[0]
    if w.dim() != 2 or w.shape[1] != E or (b is not None and b.numel() != S) or (v is not None and (v.dim() != 2 or v.shape[0] != S)):
        raise N.NativeError("soft_embed: feat [..., %d] vs w %s, bias %s, values %s"
                            % (E, tuple(w.shape), None if b is None else tuple(b.shape), None if v is None else tuple(v.shape)))
    D = E if v is None else v.shape[1]
    lead, dev = tuple(feat.shape[:-1]), feat.device
    M = feat.numel() // E
    out = torch.empty(lead + (D,), dtype=torch.float32, device=dev)
    lse = torch.empty(lead, dtype=torch.float32, device=dev) if want_lse else None
    nws = lib.tal_soft_embed_workspace_bytes(M, S, E, D)
    ws = _ws(nws, dev)
    N.check(lib.tal_soft_embed_fwd(N.ptr(feat), M, E, E, N.ptr(w), N.ptr(b), S, N.ptr(v), D, N.ptr(out), N.ptr(lse), N.ptr(ws), nws,
                                   N.stream_handle()), "tal_soft_embed_fwd")
    return (out, lse) if want_lse else out


def soft_embed_rows(x, values, want_lse=False):
    """x [..., n] (logits), values [n, D] -> out [..., D] (and lse [...]): softmax(x) . values over a materialised matrix
    (tal_soft_embed_rows); x is not modified."""
    lib = N.lib()
    x = _f32c(x, "soft_embed_rows")
    v = _f32c(values, "soft_embed_rows(values)")
    Nn = x.shape[-1]
    if v.dim() != 2 or v.shape[0] != Nn:
        raise N.NativeError("soft_embed_rows: x [..., %d] vs values %s" % (Nn, tuple(v.shape)))
    D = v.shape[1]
    lead = tuple(x.shape[:-1])
    M = x.numel() // Nn
    out = torch.empty(lead + (D,), dtype=torch.float32, device=x.device)
    lse = torch.empty(lead, dtype=torch.float32, device=x.device) if want_lse else None
    nws = lib.tal_soft_embed_rows_workspace_bytes(M, Nn, D)
    ws = _ws(nws, x.device)
    N.check(lib.tal_soft_embed_rows(N.ptr(x), M, Nn, N.ptr(v), D, N.ptr(out), N.ptr(lse), N.ptr(ws), nws, N.stream_handle()),
            "tal_soft_embed_rows")
    return (out, lse) if want_lse else out


def add_positional(x, pe):
    """x [B, U, D] + pe[:U] (PositionalEncoding.forward, tal/modules.py:63)."""
    lib = N.lib()
    x = _f32c(x, "add_positional")
    B, U, D = x.shape
    out = torch.empty_like(x)
    N.check(lib.tal_add_positional_fwd(N.ptr(x), B, U, D, N.ptr(_f32c(pe, "pe")), pe.shape[0], N.ptr(out),
                                       N.stream_handle()), "tal_add_positional_fwd")
    return out


# ------------------------------------------------------------------ WER / WDER scoring: tiled edit-distance alignment
EDIT_TAGS = ("equal", "replace", "insert", "delete")      # TAL_EDIT_TAG_* of include/tal_asrd.h; TAL_EDIT_TAG_NONE pads a pair's m + n bytes
EDIT_TAG_NONE = 255
EDIT_BUDGET_FRACTION = 0.25      # of the memory this process could still get (the K | V table's rule, system._UnalignedRun._table_fits)
EDIT_MAX_PAIRS = 65535           # pairs per tal_edit_align_fwd call


def edit_align_tile():
    """(rows, cols) of a tile of the edit-distance sweep (tal_edit_align_tile)."""
    r, c = C.c_int(), C.c_int()
    N.lib().tal_edit_align_tile(C.byref(r), C.byref(c))
    return r.value, c.value


class EditAlignment:
    """Result of edit_align for P pairs, everything on the device: stats [P, 4] int64 = (distance, path steps, equal steps, replace
    steps), dist = stats[:, 0], path (uint8, forward order; pair p owns path[path_offsets[p] : path_offsets[p + 1]] = its steps, then
    EDIT_TAG_NONE up to m + n) or None, counts [P, Ka, Kb] int64 or None.  path_offsets is host data; launches is the number of
    kernel launches the call made."""

    def __init__(self, stats, path, path_offsets, counts, launches, workspace_bytes):
        self.stats, self.path, self.path_offsets, self.counts = stats, path, path_offsets, counts
        self.launches, self.workspace_bytes = launches, workspace_bytes

    @property
    def dist(self):
        return self.stats[:, 0]

    def tags(self):
        """The paths on the host: one uint8 array of TAL_EDIT_TAG_* per pair (copies the path and the step counts)."""
        if self.path is None:
            raise N.NativeError("edit_align: the call was made with want_path=False")
        steps = self.stats[:, 1].cpu().numpy()
        flat = self.path.cpu().numpy()
        return [flat[o:o + int(k)] for o, k in zip(self.path_offsets[:-1], steps)]


def _edit_is_batch(x):
    import numpy as np
    if isinstance(x, (torch.Tensor, np.ndarray)):
        return x.ndim > 1
    return len(x) > 0 and isinstance(x[0], (list, tuple, torch.Tensor, np.ndarray))


def _edit_cat(seqs, dev, what, upper=None):
    """Ragged integer sequences (host sequences or 1-D tensors) -> one int32 device tensor + the host offset table."""
    import numpy as np
    lens = [int(s.numel()) if isinstance(s, torch.Tensor) else len(s) for s in seqs]
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    if seqs and all(isinstance(s, torch.Tensor) and s.is_cuda for s in seqs):
        for s in seqs:
            if s.dtype.is_floating_point or s.dtype == torch.bool or s.dim() != 1:
                raise N.NativeError("%s: expected 1-D integer tensors, got %s %s" % (what, s.dtype, tuple(s.shape)))
        return torch.cat([s.to(device=dev, dtype=torch.int32) for s in seqs]).contiguous(), off
    host = np.zeros(int(off[-1]), dtype=np.int64)
    for s, o, k in zip(seqs, off[:-1], lens):
        if k:
            v = np.asarray(s.cpu() if isinstance(s, torch.Tensor) else s)
            if v.ndim != 1 or v.dtype.kind not in "iu":
                raise N.NativeError("%s: expected 1-D integer sequences, got %s %s" % (what, v.dtype, v.shape))
            host[o:o + k] = v
    if host.size and (host.min() < (0 if upper is not None else -2 ** 31) or host.max() >= (upper if upper is not None else 2 ** 31)):
        raise N.NativeError("%s: values outside [%d, %d)" % (what, 0 if upper is not None else -2 ** 31, upper if upper is not None else 2 ** 31))
    return torch.from_numpy(host.astype(np.int32)).to(dev), off


def edit_align(a, b, a_labels=None, b_labels=None, n_labels=None, want_path=True, budget_bytes=None, device=None):
    """Unit-cost Levenshtein distance and the alignment of wder.align_opcodes on the device (tal_edit_align_fwd) -> EditAlignment.
    a / b: ONE pair of integer id sequences (equal words = equal ids) or two equally long lists of them; host sequences are uploaded,
    1-D device tensors are used where they are.  a_labels / b_labels (same shapes, labels 0 <= x < n_labels) ask for counts
    [P, Ka, Kb]; n_labels: an int, a (Ka, Kb) pair, or None = one more than the largest label (host labels only).
    want_path=False runs the distance sweep alone (no second table, no back-pointers, no traceback).
    A batch is cut into calls whose workspace stays within budget_bytes (default: EDIT_BUDGET_FRACTION of the memory the process can
    still get); a single pair beyond it raises NativeError before anything is launched.  Nothing is copied back to the host."""
    import numpy as np
    lib = N.lib()
    dev = torch.device(device) if device is not None else next((x.device for x in (a, b) if isinstance(x, torch.Tensor)), torch.device("cuda:0"))
    if not _edit_is_batch(a) and not _edit_is_batch(b):
        a, b = [a], [b]
        a_labels = None if a_labels is None else [a_labels]
        b_labels = None if b_labels is None else [b_labels]
    a, b = list(a), list(b)
    if len(a) != len(b):
        raise N.NativeError("edit_align: %d reference sequences vs %d hypothesis sequences" % (len(a), len(b)))
    if dev.type != "cuda":
        raise N.NativeError("edit_align: the hot path only runs on the GPU (HIP kernels); got device %s and there is deliberately no "
                            "CPU fallback (wder.levenshtein / wder.align_opcodes are the host routines)" % dev)
    if (a_labels is None) != (b_labels is None):
        raise N.NativeError("edit_align: labels are needed for both sides or for neither")
    labels = a_labels is not None
    if labels and not want_path:
        raise N.NativeError("edit_align: counts need the path (want_path=True)")
    P = len(a)
    Ka = Kb = 0
    if labels:
        if isinstance(n_labels, (tuple, list)):
            Ka, Kb = int(n_labels[0]), int(n_labels[1])
        elif n_labels is not None:
            Ka = Kb = int(n_labels)
    ids_a, a_off = _edit_cat(a, dev, "edit_align(a)")
    ids_b, b_off = _edit_cat(b, dev, "edit_align(b)")
    lab_a = lab_b = None
    if labels:
        a_labels, b_labels = list(a_labels), list(b_labels)
        if n_labels is None:
            if any(isinstance(s, torch.Tensor) and s.is_cuda for s in a_labels + b_labels):
                raise N.NativeError("edit_align: n_labels is needed with device labels")
            Ka = 1 + max([int(np.max(s)) for s in a_labels if len(s)] or [0])
            Kb = 1 + max([int(np.max(s)) for s in b_labels if len(s)] or [0])
        if Ka <= 0 or Kb <= 0 or Ka * Kb > 1 << 24:
            raise N.NativeError("edit_align: n_labels = (%d, %d): both must be positive and their product at most 2^24" % (Ka, Kb))
        lab_a, la_off = _edit_cat(a_labels, dev, "edit_align(a_labels)", Ka)
        lab_b, lb_off = _edit_cat(b_labels, dev, "edit_align(b_labels)", Kb)
        if not np.array_equal(la_off, a_off) or not np.array_equal(lb_off, b_off):
            raise N.NativeError("edit_align: every label sequence must be as long as its id sequence")
    m, n = np.diff(a_off), np.diff(b_off)
    path_off = np.zeros(P + 1, dtype=np.int64)
    np.cumsum(m + n, out=path_off[1:])
    # workspace of each pair (a call's workspace is the sum over its pairs), the budget, the cut into calls
    need = []
    for p in range(P):
        oa, ob = np.array([0, m[p]], dtype=np.int64), np.array([0, n[p]], dtype=np.int64)
        need.append(int(lib.tal_edit_align_workspace_bytes(1, oa.ctypes.data, ob.ctypes.data, int(want_path))))
    if budget_bytes is None:
        free, _ = torch.cuda.mem_get_info(dev)
        budget_bytes = EDIT_BUDGET_FRACTION * (free + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev))
    for p in range(P):
        if need[p] > budget_bytes:
            raise N.NativeError("edit_align: pair %d (m=%d, n=%d) needs a workspace of %d bytes, the budget is %d bytes; there is no host "
                                "fallback (backend=\"host\" of wder.py is the host route)" % (p, m[p], n[p], need[p], int(budget_bytes)))
    calls, p0, acc = [], 0, 0
    for p in range(P):
        if p > p0 and (acc + need[p] > budget_bytes or p - p0 == EDIT_MAX_PAIRS):
            calls.append((p0, p))
            p0, acc = p, 0
        acc += need[p]
    if P:
        calls.append((p0, P))
    stats = torch.empty((P, 4), dtype=torch.int64, device=dev)
    path = torch.empty(max(int(path_off[-1]), 1), dtype=torch.uint8, device=dev)[:int(path_off[-1])] if want_path else None
    counts = torch.empty((P, Ka, Kb), dtype=torch.int64, device=dev) if labels else None
    launches, ws_max = 0, 0
    with torch.cuda.device(dev):
        for p0, p1 in calls:
            k = p1 - p0
            oa, ob = np.ascontiguousarray(a_off[p0:p1 + 1]), np.ascontiguousarray(b_off[p0:p1 + 1])
            desc = np.zeros((k, 8), dtype=np.int64)
            nws, npath, nl = C.c_size_t(), C.c_int64(), C.c_int()
            N.check(lib.tal_edit_align_plan(k, oa.ctypes.data, ob.ctypes.data, int(want_path), desc.ctypes.data, C.byref(nws), C.byref(npath),
                                            C.byref(nl)), "tal_edit_align_plan")
            desc_dev = torch.from_numpy(desc).to(dev)
            ws = _ws(nws.value, dev)
            N.check(lib.tal_edit_align_fwd(desc.ctypes.data, N.ptr(desc_dev), k, N.ptr(ids_a), N.ptr(ids_b), N.ptr(lab_a), N.ptr(lab_b), Ka, Kb,
                                           C.c_void_p(stats.data_ptr() + 32 * p0),
                                           C.c_void_p(path.data_ptr() + int(path_off[p0])) if want_path else None,
                                           C.c_void_p(counts.data_ptr() + 8 * Ka * Kb * p0) if labels else None,
                                           N.ptr(ws), nws.value, N.stream_handle()), "tal_edit_align_fwd")
            launches += nl.value
            ws_max = max(ws_max, nws.value)
    return EditAlignment(stats, path, path_off, counts, launches, ws_max)


# ------------------------------------------------------------------ speaker turns
TURNS_MAX_HALF = 31              # TAL_TURNS_MAX_HALF: largest half window of the mode filter
SEGMENT_MEAN_CHUNK = 128         # TAL_SEGMENT_MEAN_CHUNK: rows of a chunk of segment_mean's fixed summation order
TURNS_MAX_FRAMES = 2 ** 31 - 1 - 2 * 256 - 2 * TURNS_MAX_HALF


def speaker_turns_tile():
    """(tile, max_half): frames per workgroup of the speaker-turn kernels and the largest half window (tal_speaker_turns_tile)."""
    t, h = C.c_int(), C.c_int()
    N.lib().tal_speaker_turns_tile(C.byref(t), C.byref(h))
    return t.value, h.value


class SpeakerTurns:
    """Result of speaker_turns for B items, everything on the device.  Item b owns the turns [offsets[b], offsets[b + 1]) (int64
    [B + 1]); per turn: start / end (int32, frames relative to the item, end exclusive), label (int32), purity (int32: frames of
    the turn whose raw id equals the label), embed (fp32 [turns, E], the mean of the turn's feature rows, NOT normalised -- or None
    without feat); frame_labels (int32 [N], the label of the turn that holds each frame -- or None without want_frames)."""

    def __init__(self, offsets, start, end, label, purity, embed, frame_labels):
        self.offsets, self.start, self.end, self.label, self.purity = offsets, start, end, label, purity
        self.embed, self.frame_labels = embed, frame_labels

    @property
    def num_turns(self):
        return int(self.start.numel())


def _segment_mean(feat, ranges, max_rows, check):
    lib = N.lib()
    Nf, E = feat.shape
    G = ranges.shape[0]
    out = torch.empty(G, E, dtype=torch.float32, device=feat.device)
    if G == 0:
        return out
    nws = lib.tal_segment_mean_workspace_bytes(G, max_rows, E)
    if nws == 0:
        raise N.NativeError("segment_mean: %d ranges over %d rows of width %d: the width must be a multiple of 4 in [4, 1024]" % (G, max_rows, E))
    ws = _ws(nws, feat.device)
    status = torch.empty(1, dtype=torch.int32, device=feat.device)
    N.check(lib.tal_segment_mean_fwd(N.ptr(feat), Nf, E, N.ptr(ranges), G, max_rows, N.ptr(out), N.ptr(status), N.ptr(ws), nws,
                                     N.stream_handle()), "tal_segment_mean_fwd")
    if check:
        st = int(status.item())
        if st & 1:
            raise N.NativeError("segment_mean: a range is not 0 <= start <= end <= %d" % Nf)
        if st & 2:
            raise N.NativeError("segment_mean: the ranges cover more than the %d rows their workspace was sized for" % max_rows)
    return out


def segment_mean(feat, ranges):
    """feat [N, E] fp32, ranges [G, 2] (integers, host or device; any order, overlaps allowed) -> [G, E]: out[g] = the mean of
    feat[ranges[g, 0] : ranges[g, 1]], zeros for an empty range (tal_segment_mean_fwd).  The order of every addition is fixed by the
    range and E alone (chunks of SEGMENT_MEAN_CHUNK rows counted from the range's start, added in chunk order), so the result is
    bit-identical call after call and whatever other ranges share the call.  E: a multiple of 4 up to 1024.  A range outside
    [0, N] raises.  One small device-to-host read per call (the summed range length, when the ranges live on the device, and the
    status word)."""
    feat = _f32c(feat, "segment_mean")
    if feat.dim() != 2:
        raise N.NativeError("segment_mean: feat must be [N, E], got %s" % (tuple(feat.shape),))
    if not torch.is_tensor(ranges):
        ranges = torch.as_tensor(ranges)
    if ranges.dtype.is_floating_point or ranges.dtype == torch.bool or ranges.numel() % 2 or (ranges.numel() and (ranges.dim() != 2 or ranges.shape[1] != 2)):
        raise N.NativeError("segment_mean: ranges must be integers of shape [G, 2], got %s %s" % (ranges.dtype, tuple(ranges.shape)))
    ranges = ranges.reshape(-1, 2).to(torch.int64)
    rows = int((ranges[:, 1] - ranges[:, 0]).clamp_(min=0).sum()) if ranges.numel() else 0
    return _segment_mean(feat, ranges.to(feat.device).contiguous(), rows, True)


def speaker_turns(ids, num_ids, offsets=None, smooth=0, min_frames=1, feat=None, want_frames=False):
    """Per-frame speaker ids -> who-spoke-when turns on the device (tal_speaker_turns_fwd) -> SpeakerTurns.

    ids: int32 device tensor, the frames of B items back to back (any shape: it is flattened); offsets: B + 1 ascending host integers
    from 0 to ids.numel() (list / array / CPU tensor; a device tensor is copied to the host), item b = ids[offsets[b] : offsets[b + 1]],
    an item may be empty; None = one item.  Every id must lie in [0, num_ids): one outside raises NativeError and nothing is returned.
      1. mode filter, half window `smooth` in [0, 31]: each frame takes the most frequent id of [t - smooth, t + smooth] clipped to
         its item; among ids tied for the most, the frame's own id if it is one of them, else the smallest.
      2. maximal runs of equal filtered ids inside an item; a run shorter than `min_frames` takes the label of the nearest run of at
         least min_frames frames before it in the item, else of the nearest such run after it; an item without such a run keeps its
         runs; adjacent runs of equal label merge into turns.
      3. per turn start / end / label / purity, and with feat [N, E] (fp32, E a multiple of 4 up to 1024) embed = the mean of the
         turn's rows (segment_mean's fixed order; not normalised -- torch.nn.functional.normalize is the caller's line).
    Integer outputs are exact.  One device-to-host read per call (the number of turns with the status word, 16 bytes); the
    per-turn tensors are views of that length into buffers sized for the bound (one turn per frame)."""
    lib = N.lib()
    N.require_cuda(ids, "speaker_turns")
    if ids.dtype != torch.int32:
        raise N.NativeError("speaker_turns: ids must be int32 (SDModel.speaker_ids' ids), got %s" % ids.dtype)
    for name, v, lo in (("num_ids", num_ids, 1), ("smooth", smooth, 0), ("min_frames", min_frames, 1)):
        if isinstance(v, bool) or int(v) != v or int(v) < lo or int(v) > 2 ** 31 - 1:
            raise N.NativeError("speaker_turns: %s=%r must be an integer >= %d" % (name, v, lo))
    if int(smooth) > TURNS_MAX_HALF:
        raise N.NativeError("speaker_turns: smooth=%d outside [0, %d]" % (smooth, TURNS_MAX_HALF))
    dev = ids.device
    ids = ids.contiguous().reshape(-1)
    n = ids.numel()
    import numpy as np
    if offsets is None:
        off = np.array([0, n], np.int64)
    else:
        off = np.ascontiguousarray((offsets.detach().cpu() if torch.is_tensor(offsets) else torch.as_tensor(np.asarray(offsets))).numpy()
                                   .astype(np.int64).reshape(-1))
    B = len(off) - 1
    if B < 0 or off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
        raise N.NativeError("speaker_turns: offsets must ascend from 0 to ids.numel() = %d" % n)
    if n > TURNS_MAX_FRAMES or B > 2 ** 31 - 2:
        raise N.NativeError("speaker_turns: %d frames in %d items (at most %d frames per call)" % (n, B, TURNS_MAX_FRAMES))
    if feat is not None:
        feat = _f32c(feat, "speaker_turns(feat)")
        if feat.dim() < 2 or feat.numel() != n * feat.shape[-1] or feat.device != dev:
            raise N.NativeError("speaker_turns: feat %s does not hold one row per frame (%d frames on %s)" % (tuple(feat.shape), n, dev))
        feat = feat.reshape(n, feat.shape[-1])
        if feat.shape[1] % 4 or not 4 <= feat.shape[1] <= 1024:
            raise N.NativeError("speaker_turns: feat rows of %d floats (a multiple of 4 in [4, 1024])" % feat.shape[1])
    off_dev = torch.from_numpy(off).to(dev)
    buf = torch.empty(4, max(n, 1), dtype=torch.int32, device=dev)
    frames = torch.empty(n, dtype=torch.int32, device=dev) if want_frames else None
    ranges = torch.empty(n, 2, dtype=torch.int64, device=dev) if feat is not None else None      # the turns' rows of feat
    meta = torch.zeros(B + 2, dtype=torch.int64, device=dev)      # turn_offsets [B + 1], then the status word
    status = meta[B + 1:].view(torch.int32)
    nws = lib.tal_speaker_turns_workspace_bytes(n)
    ws = _ws(nws, dev)
    N.check(lib.tal_speaker_turns_fwd(N.ptr(ids), off.ctypes.data, N.ptr(off_dev), B, int(num_ids), int(smooth), int(min_frames),
                                      N.ptr(buf[0]), N.ptr(buf[1]), N.ptr(buf[2]), N.ptr(buf[3]), N.ptr(frames), N.ptr(ranges), N.ptr(meta), N.ptr(status),
                                      N.ptr(ws), nws, N.stream_handle()), "tal_speaker_turns_fwd")
    total, st = meta[B:].tolist()      # the one read-back
    if st & 1:
        raise N.NativeError("speaker_turns: an id lies outside [0, %d)" % num_ids)
    start, end, label, purity = (buf[i, :total] for i in range(4))
    embed = None
    if feat is not None:
        # (the ranges are the call's own turns: inside [0, n] and n rows together, so the status word needs no second read)
        embed = _segment_mean(feat, ranges[:total], n, False)
    return SpeakerTurns(meta[:B + 1], start, end, label, purity, embed, frames)
