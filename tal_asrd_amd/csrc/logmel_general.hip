// Log-mel front-end for any sample rate and mel count: LogMelSpec(sr, n_mels) (tal/asr/models.py:22-53) with runtime shapes
//   reflect-pad n_fft / 2 | frames of n_fft @ hop | the window as given | one-sided n_fft-point DFT (n_fft / 2 + 1 bins) |
//   re^2+im^2 | the filterbank as given ([n_fft / 2 + 1, n_mels], any values) | log(. + eps) | optionally minus ONE global mean.
// Same precision policy as csrc/logmel.hip: window x sample, the DFT and the power in float64 (near-silent frames); the mel
// projection and the log in float32.  n_fft 32..2048 (odd or even), hop 1..n_fft, n_mels 1..256.
//
// One workgroup = F (32, or 16 where 32 frames' samples do not fit in LDS) consecutive frames of one batch item.  The
// (F-1) * hop + n_fft samples they span are staged once into LDS, reflect indexing resolved at load.  The WINDOWED frame y is
// folded while the A operand is formed (exact for any window: the basis, not the window, carries the symmetry):
//   Re X[k] =  sum_{n=0}^{M-1} s[n] cos(2 pi k n / N),   s[n] = y[n] + y[N-n]   (1 <= n < N/2),  y[0] (n = 0),  y[N/2] (even N)
//   Im X[k] = -sum_{n=0}^{M-1} d[n] sin(2 pi k n / N),   d[n] = y[n] - y[N-n]   (the n = 0 and n = N/2 basis rows are zero)
// with M = N/2 + 1 terms (floor), padded to MP = a multiple of 4.  The transform is then a [F x MP] . [MP x 16 bins] contraction
// per bin tile on v_mfma_f64_16x16x4_f64 against a cos / -sin basis kept in the plan ([tile][n][16 bins][cos | -sin]).
// Bin tiles are processed in chunks that fit an LDS power tile; after each chunk every (frame, filter) output adds the chunk's
// bins of its filter's support to a float32 accumulator in LDS, always in the same order (results do not depend on timing).
// Per-workgroup float64 partial sums feed the mean / subtract kernels of csrc/logmel.hip.
#include <math.h>

#include <cstddef>
#include <cstring>
#include <vector>

#include "common.h"

namespace tal {

constexpr int GM_NFFT_MIN = 32, GM_NFFT_MAX = 2048, GM_NMEL_MAX = 256;
constexpr int GM_MAGIC = 0x4c4d4731;                  // plan header word 0
constexpr size_t GM_LDS_MAX = 160 * 1024 - 256;       // dynamic LDS one workgroup may take (the rest: the kernel's static words)
constexpr size_t GM_LDS_SOFT = 64 * 1024;             // preferred ceiling (two workgroups per CU) when the chunking allows it

// Plan layout (byte offsets), a function of (n_fft, n_mels) alone.  Header: {magic, n_fft, hop, n_mels} in the first 64 bytes.
struct GLayout {
    int M, MP, nbin, ntile;
    size_t win, basis, lo, cnt, off, wc, bytes;
};
__host__ __device__ inline size_t gm_al(size_t x) { return (x + 255) & ~(size_t)255; }
__host__ __device__ inline GLayout gm_layout(int N, int nm) {
    GLayout g;
    g.M = N / 2 + 1;
    g.MP = (g.M + 3) & ~3;
    g.nbin = N / 2 + 1;
    g.ntile = (g.nbin + 15) / 16;
    g.win = 256;
    g.basis = gm_al(g.win + (size_t)N * 4);
    g.lo = gm_al(g.basis + (size_t)g.ntile * g.MP * 16 * 16);
    g.cnt = gm_al(g.lo + (size_t)nm * 4);
    g.off = gm_al(g.cnt + (size_t)nm * 4);
    g.wc = gm_al(g.off + (size_t)nm * 4);
    g.bytes = gm_al(g.wc + (size_t)g.nbin * nm * 4);
    return g;
}

struct GArgs {
    const char* plan;
    int64_t L, T;
    int N, hop, nm, M, MP, ntile;
    int ct;          // bin tiles per chunk
    int ns;          // staged samples: (F - 1) * hop + N
    float eps;
};

// LDS use of one workgroup of F frames: the window halves [2][MP], the samples, the power chunk [F][ct * 16], the accumulators [F][nm]
static size_t gm_lds_bytes(int F, int MP, int ns, int ct, int nm) {
    return ((size_t)2 * MP + ns + (size_t)F * ct * 16 + (size_t)F * nm) * sizeof(float);
}

template <bool TWO, typename AT>
__global__ __launch_bounds__(256) void logmel_general_kernel(GArgs a, const AT* __restrict__ audio, float* __restrict__ out,
                                                             double* __restrict__ partial) {
    constexpr int F = TWO ? 32 : 16;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = wave_id();
    const int b = blockIdx.y;
    const int64_t f0 = (int64_t)blockIdx.x * F;
    const int nm = a.nm;
    const int nout = F * nm;
    const GLayout g = gm_layout(a.N, nm);
    {
        // a plan built for another shape: this workgroup's outputs (the caller's shape, in bounds) and partial sum become NaN
        const int* hdr = reinterpret_cast<const int*>(a.plan);
        if (hdr[0] != GM_MAGIC || hdr[1] != a.N || hdr[2] != a.hop || hdr[3] != nm) {
            for (int idx = tid; idx < nout; idx += 256) {
                const int frame = idx / nm;
                if (f0 + frame < a.T) out[((int64_t)b * a.T + f0) * nm + idx] = __builtin_nanf("");
            }
            if (tid == 0) partial[(int64_t)b * gridDim.x + blockIdx.x] = __builtin_nan("");
            return;
        }
    }
    float* wa = lds;                    // wa[n] = w[n]     (n < M; 0 past it)
    float* wb = wa + a.MP;              // wb[n] = w[N - n] (1 <= n < N/2; 0 elsewhere)
    float* samp = wb + a.MP;
    float* P = samp + a.ns;
    float* macc = P + F * a.ct * 16;
    const float* win = reinterpret_cast<const float*>(a.plan + g.win);
    for (int n = tid; n < a.MP; n += 256) {
        wa[n] = n < a.M ? win[n] : 0.f;
        wb[n] = (n >= 1 && 2 * n < a.N) ? win[a.N - n] : 0.f;
    }
    const AT* ab = audio + (int64_t)b * a.L;
    const int64_t p0 = f0 * a.hop - a.N / 2;
    for (int i = tid; i < a.ns; i += 256) {
        int64_t p = p0 + i;
        if (p < 0) p = -p;                       // reflect (no edge repeat), as torch.stft pad_mode='reflect'; L > N/2 keeps it in range
        if (p >= a.L) p = 2 * (a.L - 1) - p;
        p = p < 0 ? 0 : (p >= a.L ? a.L - 1 : p);    // frames past T (tail block) only
        samp[i] = (float)ab[p];
    }
    for (int idx = tid; idx < nout; idx += 256) macc[idx] = 0.f;
    __syncthreads();

    typedef double f64x4 __attribute__((ext_vector_type(4)));
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    const f64x2* basis = reinterpret_cast<const f64x2*>(a.plan + g.basis);
    const int* mlo = reinterpret_cast<const int*>(a.plan + g.lo);
    const int* mcnt = reinterpret_cast<const int*>(a.plan + g.cnt);
    const int* moff = reinterpret_cast<const int*>(a.plan + g.off);
    const float* wc = reinterpret_cast<const float*>(a.plan + g.wc);
    const int fi = lane & 15;   // frame (A row) / bin (B col) inside a 16x16 tile
    const int kq = lane >> 4;   // which of the 4 k's of a 16x16x4 step
    const float* s0 = samp + fi * a.hop;
    const float* s1 = s0 + 16 * a.hop;
    const int pc = a.ct * 16;
    for (int t0 = 0; t0 < a.ntile; t0 += a.ct) {
        const int t1 = t0 + a.ct < a.ntile ? t0 + a.ct : a.ntile;
        for (int j = t0 + w; j < t1; j += 4) {
            f64x4 re0 = {0., 0., 0., 0.}, im0 = re0, re1 = re0, im1 = re0;
            const f64x2* bp = basis + ((int64_t)j * a.MP + kq) * 16 + fi;
            for (int k = 0; k < a.MP; k += 4) {
                const int n = k + kq;                               // n < MP <= N/2 + 4 <= N - 1: inside the frame
                const int nb = (n >= 1 && 2 * n < a.N) ? a.N - n : n;
                const double wan = (double)wa[n], wbn = (double)wb[n];
                const f64x2 bb = bp[(int64_t)k * 16];
                const double u0 = wan * (double)s0[n], v0 = wbn * (double)s0[nb];
                re0 = __builtin_amdgcn_mfma_f64_16x16x4f64(u0 + v0, bb.x, re0, 0, 0, 0);
                im0 = __builtin_amdgcn_mfma_f64_16x16x4f64(u0 - v0, bb.y, im0, 0, 0, 0);
                if constexpr (TWO) {
                    const double u1 = wan * (double)s1[n], v1 = wbn * (double)s1[nb];
                    re1 = __builtin_amdgcn_mfma_f64_16x16x4f64(u1 + v1, bb.x, re1, 0, 0, 0);
                    im1 = __builtin_amdgcn_mfma_f64_16x16x4f64(u1 - v1, bb.y, im1, 0, 0, 0);
                }
            }
            // f64 16x16 C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg
            const int col = (j - t0) * 16 + fi;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int frame = kq + 4 * e;
                P[frame * pc + col] = (float)(re0[e] * re0[e] + im0[e] * im0[e]);
                if constexpr (TWO) P[(frame + 16) * pc + col] = (float)(re1[e] * re1[e] + im1[e] * im1[e]);
            }
        }
        __syncthreads();
        // this chunk's bins [t0 * 16, t1 * 16) of every filter's support, added in bin order (bins past n_fft / 2 are never in a support)
        const int c0 = t0 * 16, c1 = t1 * 16;
        for (int idx = tid; idx < nout; idx += 256) {
            const int frame = idx / nm;
            const int m = idx - frame * nm;
            const int lo = mlo[m], hi = lo + mcnt[m];
            const int b0 = lo > c0 ? lo : c0, b1 = hi < c1 ? hi : c1;
            if (b0 < b1) {
                const float* pr = P + frame * pc - c0;
                const float* wm = wc + moff[m] - lo;
                float s = macc[idx];
                for (int k = b0; k < b1; ++k) s = fmaf(pr[k], wm[k], s);
                macc[idx] = s;
            }
        }
        __syncthreads();
    }

    double local = 0.0;
    float* ob = out + ((int64_t)b * a.T + f0) * nm;
    for (int idx = tid; idx < nout; idx += 256) {
        const int frame = idx / nm;
        const float v = logf(macc[idx] + a.eps);
        if (f0 + frame < a.T) {
            ob[idx] = v;
            local += (double)v;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off, 64);
    if (lane == 0) red[w] = local;
    __syncthreads();
    if (tid == 0) partial[(int64_t)b * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

static bool gm_shape_ok(int N, int hop, int nm) {
    return N >= GM_NFFT_MIN && N <= GM_NFFT_MAX && hop >= 1 && hop <= N && nm >= 1 && nm <= GM_NMEL_MAX;
}

// frames per workgroup and bin tiles per chunk for a shape: 32 frames where their samples and a 4-tile chunk fit, else 16 (always
// fits: 2048-point frames at hop 2048 with 256 filters take 152 KiB with one tile per chunk); chunks as large as LDS allows,
// kept under 64 KiB when that still leaves 4 tiles (one per wave) per chunk
struct GConfig {
    int F, ct, ns;
    size_t lds;
};
static GConfig gm_config(int N, int hop, int nm) {
    const GLayout g = gm_layout(N, nm);
    GConfig c;
    const int tmin = g.ntile < 4 ? g.ntile : 4;
    c.F = gm_lds_bytes(32, g.MP, 31 * hop + N, tmin, nm) <= GM_LDS_MAX ? 32 : 16;
    c.ns = (c.F - 1) * hop + N;
    const size_t fixed = gm_lds_bytes(c.F, g.MP, c.ns, 0, nm);
    const size_t per_tile = (size_t)c.F * 16 * sizeof(float);
    size_t ct = (GM_LDS_MAX - fixed) / per_tile;
    if (fixed < GM_LDS_SOFT && (GM_LDS_SOFT - fixed) / per_tile >= (size_t)tmin) ct = (GM_LDS_SOFT - fixed) / per_tile;
    c.ct = ct < (size_t)g.ntile ? (int)ct : g.ntile;
    c.lds = gm_lds_bytes(c.F, g.MP, c.ns, c.ct, nm);
    return c;
}

template <bool TWO, typename AT>
static int gm_launch(const GArgs& a, const GConfig& c, int B, int64_t nblk, const AT* audio, float* out, double* partial, hipStream_t s) {
    auto kern = logmel_general_kernel<TWO, AT>;
    static bool attr_set = false;      // (the largest size any shape takes; racing first calls set the same value)
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)GM_LDS_MAX) !=
            hipSuccess) {
            set_error("tal_logmel_general_fwd: cannot reserve %zu bytes of LDS", GM_LDS_MAX);
            return TAL_EHIP;
        }
        attr_set = true;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk, (unsigned)B), dim3(256), c.lds, s, a, audio, out, partial);
    TAL_CHECK_LAUNCH("tal_logmel_general_fwd");
    return TAL_OK;
}

}  // namespace tal

using namespace tal;

extern "C" int64_t tal_logmel_frames(int64_t L, int hop) { return hop >= 1 && L >= 0 ? 1 + L / hop : 0; }

extern "C" size_t tal_logmel_general_plan_bytes(int n_fft, int n_mels) {
    if (!gm_shape_ok(n_fft, 1, n_mels)) return 0;
    return gm_layout(n_fft, n_mels).bytes;
}

extern "C" int tal_logmel_general_plan_init(const float* window, int n_fft, int hop, const float* fb, int n_mels, void* plan,
                                            void* stream) {
    TAL_CHECK_ARG(window && fb && plan, "tal_logmel_general_plan_init: null pointer");
    TAL_CHECK_ARG(n_fft >= GM_NFFT_MIN && n_fft <= GM_NFFT_MAX, "tal_logmel_general_plan_init: n_fft=%d outside %d..%d", n_fft,
                  GM_NFFT_MIN, GM_NFFT_MAX);
    TAL_CHECK_ARG(hop >= 1 && hop <= n_fft, "tal_logmel_general_plan_init: hop=%d outside 1..n_fft (%d)", hop, n_fft);
    TAL_CHECK_ARG(n_mels >= 1 && n_mels <= GM_NMEL_MAX, "tal_logmel_general_plan_init: n_mels=%d outside 1..%d", n_mels, GM_NMEL_MAX);
    hipStream_t s = (hipStream_t)stream;
    const int N = n_fft, nm = n_mels;
    const GLayout g = gm_layout(N, nm);
    std::vector<float> hwin(N), hfb((size_t)g.nbin * nm);
    if (hipMemcpyAsync(hwin.data(), window, (size_t)N * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(hfb.data(), fb, hfb.size() * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        set_error("tal_logmel_general_plan_init: cannot read window/fb from the device");
        return TAL_EHIP;
    }
    std::vector<char> buf(g.bytes, 0);
    char* hp = buf.data();
    const int hdr[4] = {GM_MAGIC, N, hop, nm};
    memcpy(hp, hdr, sizeof(hdr));
    memcpy(hp + g.win, hwin.data(), (size_t)N * sizeof(float));
    double* bs = reinterpret_cast<double*>(hp + g.basis);
    const double two_pi = 6.283185307179586476925286766559;
    for (int j = 0; j < g.ntile; ++j)
        for (int n = 0; n < g.MP; ++n)
            for (int c = 0; c < 16; ++c) {
                const int bin = j * 16 + c;
                double re = 0.0, im = 0.0;
                if (bin < g.nbin && n < g.M) {
                    const int64_t ph = ((int64_t)bin * n) % N;       // exact phase reduction
                    const double ang = two_pi * (double)ph / (double)N;
                    re = cos(ang);
                    im = (n == 0 || 2 * n == N) ? 0.0 : -sin(ang);  // d[0], d[N/2] are not differences of a pair
                }
                bs[(((size_t)j * g.MP + n) * 16 + c) * 2 + 0] = re;
                bs[(((size_t)j * g.MP + n) * 16 + c) * 2 + 1] = im;
            }
    int* lo = reinterpret_cast<int*>(hp + g.lo);
    int* cnt = reinterpret_cast<int*>(hp + g.cnt);
    int* off = reinterpret_cast<int*>(hp + g.off);
    float* wc = reinterpret_cast<float*>(hp + g.wc);
    int at = 0;
    for (int m = 0; m < nm; ++m) {
        int l = -1, h = -1;
        for (int k = 0; k < g.nbin; ++k)
            if (hfb[(size_t)k * nm + m] != 0.f) {
                if (l < 0) l = k;
                h = k;
            }
        lo[m] = l < 0 ? 0 : l;
        cnt[m] = l < 0 ? 0 : h - l + 1;      // (a filter with empty support: log(eps))
        off[m] = at;
        for (int i = 0; i < cnt[m]; ++i) wc[at + i] = hfb[(size_t)(l + i) * nm + m];
        at += cnt[m];
    }
    if (hipMemcpyAsync(plan, hp, g.bytes, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        set_error("tal_logmel_general_plan_init: cannot upload the plan");
        return TAL_EHIP;
    }
    return TAL_OK;
}

extern "C" size_t tal_logmel_general_workspace_bytes(int n_fft, int hop, int B, int64_t L) {
    if (hop < 1 || B < 1 || L < 0) return 0;
    (void)n_fft;
    const int64_t T = 1 + L / hop;
    return (size_t)(B * cdiv(T, 16) + 4) * sizeof(double);     // (16-frame workgroups: the most partial sums any shape writes)
}

extern "C" int tal_logmel_general_fwd(const void* plan, int n_fft, int hop, int n_mels, const void* audio, int audio_is_f16, int B,
                                      int64_t L, float eps, int subtract_mean, float* out, float* mean_out, double* sum_out,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "tal_logmel_general_fwd";
    TAL_CHECK_ARG(plan && audio && out && workspace, "%s: null pointer", what);
    TAL_CHECK_ARG(n_fft >= GM_NFFT_MIN && n_fft <= GM_NFFT_MAX, "%s: n_fft=%d outside %d..%d", what, n_fft, GM_NFFT_MIN, GM_NFFT_MAX);
    TAL_CHECK_ARG(hop >= 1 && hop <= n_fft, "%s: hop=%d outside 1..n_fft (%d)", what, hop, n_fft);
    TAL_CHECK_ARG(n_mels >= 1 && n_mels <= GM_NMEL_MAX, "%s: n_mels=%d outside 1..%d", what, n_mels, GM_NMEL_MAX);
    TAL_CHECK_ARG(B > 0 && L > n_fft / 2, "%s: need B>0 and L>%d (n_fft/2) for reflect padding (L=%lld)", what, n_fft / 2,
                  (long long)L);
    TAL_CHECK_ARG(!audio_is_f16 || (reinterpret_cast<uintptr_t>(audio) & 1) == 0, "%s: fp16 audio must be 2-byte aligned", what);
    // torch.stft's count over the padded signal, 1 + (L + 2 (N/2) - N) / hop: 1 + L / hop for even N, one frame less for odd N when
    // hop divides L (the last frame would reach past the padding)
    const int64_t T = 1 + (L - (n_fft & 1)) / hop;
    const GConfig c = gm_config(n_fft, hop, n_mels);
    const int64_t nblk = cdiv(T, c.F);
    TAL_CHECK_ARG(c.ct >= 1 && c.lds <= GM_LDS_MAX, "%s: no LDS layout for n_fft=%d hop=%d n_mels=%d", what, n_fft, hop, n_mels);
    TAL_CHECK_ARG(nblk < (int64_t)1 << 31 && B < 65536, "%s: %lld frames x %d items is too many workgroups", what, (long long)T, B);
    const size_t need = tal_logmel_general_workspace_bytes(n_fft, hop, B, L);
    if (workspace_bytes < need) {
        set_error("%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
        return TAL_ENOMEM;
    }
    hipStream_t s = (hipStream_t)stream;
    const GLayout g = gm_layout(n_fft, n_mels);
    GArgs a;
    a.plan = reinterpret_cast<const char*>(plan);
    a.L = L;
    a.T = T;
    a.N = n_fft;
    a.hop = hop;
    a.nm = n_mels;
    a.M = g.M;
    a.MP = g.MP;
    a.ntile = g.ntile;
    a.ct = c.ct;
    a.ns = c.ns;
    a.eps = eps;
    const int64_t nparts = (int64_t)B * nblk;
    double* partial = reinterpret_cast<double*>(workspace);
    float* mean_ws = reinterpret_cast<float*>(partial + nparts + 2);
    int rc;
    {
        // algorithmic HBM bytes: read L samples, write T * n_mels floats per item
        ProfScope prof(PROF_LOGMEL, (double)B * ((double)L * (audio_is_f16 ? 2.0 : 4.0) + (double)T * n_mels * 4.0), s);
        if (audio_is_f16)
            rc = c.F == 32 ? gm_launch<true>(a, c, B, nblk, reinterpret_cast<const _Float16*>(audio), out, partial, s)
                           : gm_launch<false>(a, c, B, nblk, reinterpret_cast<const _Float16*>(audio), out, partial, s);
        else
            rc = c.F == 32 ? gm_launch<true>(a, c, B, nblk, reinterpret_cast<const float*>(audio), out, partial, s)
                           : gm_launch<false>(a, c, B, nblk, reinterpret_cast<const float*>(audio), out, partial, s);
    }
    if (rc != TAL_OK) return rc;
    return launch_logmel_mean(partial, nparts, (double)B * (double)T * (double)n_mels, mean_out, sum_out, mean_ws, subtract_mean, out,
                              (int64_t)B * T * n_mels, s, what);
}
