// Grouped temporal convolutions of the TDS encoder at ANY kernel size k (TDS(..., kernel_size=k), tal/asr/models.py:299,354):
//
//   stride-2 "resize" conv, padding 0 ............ tal/asr/models.py:363-364    1 <= k <= TAL_GCONV_MAX_K, T_in >= k
//   TDSBlock grouped conv + ReLU + ReZero ......... tal/asr/models.py:304-308,329  odd k, padding k / 2
//
// Exact fp32 on the vector ALU, k a runtime value.  Every output starts from its bias and takes one fmaf per product, input
// channel outer and tap inner: the order of gconv_kernel, gconv_generic_kernel and gconv_s2_c1_kernel (csrc/gconv.hip), so at
// k = 21 the results equal tal_gconv_s2_fwd / tal_gconv_res_fwd bit for bit.  Three kernels:
//   gconv_k_kernel     the encoder's per-group widths (10 -> 14, 14 -> 18 resize; 10 / 14 / 18 block): gconv_kernel's scheme with
//                      a runtime tap count -- a [GB groups x C/G channels] x [tile * stride + k - 1] slab of x in LDS, channel-major,
//                      odd row pitch; a lane owns R time steps of all C_out/G channels of one group, so a group's weights are
//                      wave-uniform and come through the scalar unit while the x taps come from LDS;
//   gconv_k_c1_kernel  the first resize conv (1 mel bin -> 10 channels per group): store-bound, so gconv_s2_c1_kernel's channel-major
//                      lanes (a wave stores 256 contiguous bytes); a lane's k weights sit in LDS ([k][channels]: conflict-free);
//   gconv_k_any_kernel any other per-group width: one thread per output element (small models, unit tests).
// No LDS-DMA fills, no allocation, no synchronisation; 64-bit element offsets throughout.
#include "common.h"

namespace tal {

template <int CIG, int COG, int STRIDE, int GB, int TT, bool RESID>
__global__ __launch_bounds__(256) void gconv_k_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                     const float* __restrict__ bias, float alpha, float* __restrict__ y,
                                                     int64_t T_in, int64_t T_out, int C_in, int C_out, int ks) {
    const int pad = RESID ? ks / 2 : 0;
    const int tin = (TT - 1) * STRIDE + ks;       // input rows a tile reads
    const int tinp = tin | 1;                     // odd pitch: conflict-free transposing store and time-walking reads
    constexpr int WPG = GB >= 4 ? 1 : 4 / GB;     // waves per group (GB < 4: they split the time tile)
    constexpr int TW = TT / WPG;
    constexpr int R = TW / 64;
    static_assert(TW % 64 == 0 && R >= 1, "time tile per wave must be a multiple of 64");
    constexpr int CH = GB * CIG;
    static_assert(CH % 4 == 0, "a group slab must be a whole number of 16-byte columns");
    constexpr int CH4 = CH / 4;
    extern __shared__ __attribute__((aligned(16))) float xs[];  // [CH][tinp]

    const int b = blockIdx.z;
    const int g0 = blockIdx.y * GB;
    const int64_t t0 = (int64_t)blockIdx.x * TT;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = wave_id();

    const float* xb = x + (int64_t)b * T_in * C_in + g0 * CIG;
    const int64_t tin0 = t0 * STRIDE - pad;
    // slab: 16-byte loads, four in flight per thread (clamped address + select), zero rows outside [0, T_in)
    const int nv = tin * CH4;
    constexpr int UNR = 4;
    for (int base = 0; base < nv; base += 256 * UNR) {
        f32x4 v[UNR];
        int tiv[UNR], cv[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int idx = base + u * 256 + tid;
            const int ti = idx / CH4;
            tiv[u] = idx < nv ? ti : -1;
            cv[u] = (idx - ti * CH4) * 4;
            const int64_t t = tin0 + ti;
            const bool in = idx < nv && t >= 0 && t < T_in;
            const int64_t tc = in ? t : 0;
            const f32x4 ld = *reinterpret_cast<const f32x4*>(xb + tc * C_in + (idx < nv ? cv[u] : 0));
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            v[u] = in ? ld : z;
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            if (tiv[u] >= 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) xs[(cv[u] + q) * tinp + tiv[u]] = v[u][q];
            }
    }
    __syncthreads();

    const int part = w % WPG;
    const int tl0 = part * TW + lane;
    for (int gl = w / WPG; gl < GB; gl += 4 / WPG) {
        const int g = g0 + gl;
        float acc[R][COG];
#pragma unroll
        for (int co = 0; co < COG; ++co) {
            const float bv = bias[g * COG + co];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r][co] = bv;
        }
        const float* wg = wp + (int64_t)g * CIG * ks * COG;
        const float* xl = xs + gl * CIG * tinp + tl0 * STRIDE;
#pragma unroll 1
        for (int ci = 0; ci < CIG; ++ci) {
            const float* wc = wg + ci * ks * COG;
            const float* xc = xl + ci * tinp;
#pragma unroll 3
            for (int k = 0; k < ks; ++k) {
                float xv[R];
#pragma unroll
                for (int r = 0; r < R; ++r) xv[r] = xc[r * 64 * STRIDE + k];
#pragma unroll
                for (int co = 0; co < COG; ++co) {
                    const float wv = wc[k * COG + co];
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[r][co] = fmaf(wv, xv[r], acc[r][co]);
                }
            }
        }
        float* yb = y + (int64_t)b * T_out * C_out + g * COG;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t t = t0 + tl0 + 64 * r;
            if (t < T_out) {
#pragma unroll
                for (int co = 0; co < COG; ++co) {
                    float v = acc[r][co];
                    if (RESID) {
                        const float xin = xs[(gl * CIG + co) * tinp + tl0 + 64 * r + pad];
                        v = xin + alpha * fmaxf(v, 0.f);
                    }
                    yb[t * C_out + co] = v;
                }
            }
        }
    }
}

// First resize conv, 1 input channel per group -> COG outputs, stride 2.  A lane owns one output channel and walks the tile's
// time axis four steps at a time; the mel slab sits in LDS time-major ([row][NG groups]: lanes of one group read the same word),
// the lane's k weights behind it ([k][NC]: consecutive lanes, consecutive words).
template <int COG, int NG, int TT>
__global__ __launch_bounds__(256) void gconv_k_c1_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                        const float* __restrict__ bias, float* __restrict__ y, int64_t T_in,
                                                        int64_t T_out, int C_in, int C_out, int ks) {
    constexpr int NC = NG * COG;
    static_assert(NC <= 256 && NG % 4 == 0 && TT % 4 == 0, "shape");
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tin = (TT - 1) * 2 + ks;            // the last step of the tile reads row (TT - 1) * 2 + ks - 1
    float* xs = sm;                               // [tin][NG]
    float* wl = sm + tin * NG;                    // [ks][NC]
    const int b = blockIdx.z, g0 = blockIdx.y * NG;
    const int64_t t0 = (int64_t)blockIdx.x * TT;
    const int tid = threadIdx.x;
    const float* xb = x + (int64_t)b * T_in * C_in + g0;
    for (int i = tid; i < tin * (NG / 4); i += 256) {
        const int r = i / (NG / 4), c = (i - r * (NG / 4)) * 4;
        int64_t t = t0 * 2 + r;
        t = t < T_in ? t : T_in - 1;              // rows past the end feed outputs past T_out only
        *reinterpret_cast<f32x4*>(xs + r * NG + c) = *reinterpret_cast<const f32x4*>(xb + t * C_in + c);
    }
    // packed weight layout [G][1][k][COG]
    for (int i = tid; i < ks * NC; i += 256) {
        const int k = i / NC, c = i - k * NC;
        wl[i] = wp[((int64_t)(g0 + c / COG) * ks + k) * COG + c % COG];
    }
    __syncthreads();
    if (tid >= NC) return;
    const int ch = g0 * COG + tid;
    const float bv = bias[ch];
    const float* xc = xs + tid / COG;
    const float* wc = wl + tid;
    float* yc = y + (int64_t)b * T_out * C_out + ch;
    for (int tl = 0; tl < TT && t0 + tl < T_out; tl += 4) {
        float acc[4] = {bv, bv, bv, bv};
        const float* xt = xc + 2 * tl * NG;
#pragma unroll 3
        for (int k = 0; k < ks; ++k) {
            const float wv = wc[k * NC];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = fmaf(wv, xt[(2 * q + k) * NG], acc[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t t = t0 + tl + q;
            if (t < T_out) yc[t * C_out] = acc[q];
        }
    }
}

// Any per-group width: one thread per output element (gconv_generic_kernel with a runtime tap count; taps outside [0, T_in) skipped).
template <bool RESID>
__global__ __launch_bounds__(256) void gconv_k_any_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                         const float* __restrict__ bias, float alpha, float* __restrict__ y,
                                                         int64_t T_in, int64_t T_out, int C_in, int C_out, int cig, int cog,
                                                         int stride, int ks, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C_out);
    const int64_t bt = i / C_out;
    const int64_t t = bt % T_out;
    const int64_t b = bt / T_out;
    const int g = c / cog, co = c - g * cog;
    const int pad = RESID ? ks / 2 : 0;
    float acc = bias[c];
    const float* xb = x + b * T_in * C_in + g * cig;
    const float* wg = wp + (int64_t)g * cig * ks * cog + co;
    for (int ci = 0; ci < cig; ++ci)
        for (int k = 0; k < ks; ++k) {
            const int64_t ti = t * stride - pad + k;
            if (ti >= 0 && ti < T_in) acc = fmaf(wg[((int64_t)ci * ks + k) * cog], xb[ti * C_in + ci], acc);
        }
    if (RESID) acc = x[(b * T_in + t) * C_in + c] + alpha * fmaxf(acc, 0.f);
    y[i] = acc;
}

namespace {

// one planned launch (csrc/gconv_plan.h) on this file's kernels; (CIG, COG, STRIDE, GB, TT, RESID) of gconv_k_kernel written once
#define GCONV_K_SPECS(X) X(10, 14, 2, 4, 128, false) X(14, 18, 2, 2, 128, false) X(10, 10, 1, 2, 256, true) X(14, 14, 1, 2, 256, true) X(18, 18, 1, 2, 256, true)

int launch_planned_k(const GconvCall& c, const float* x, const float* wp, const float* bias, float alpha, float* y, hipStream_t s) {
    const GconvLaunch p = gconv_plan(c);
    if (p.refusal) return gconv_refused(c, p.refusal);
    if (p.grid_x == 0) return TAL_OK;
    const dim3 grid(p.grid_x, p.grid_y, p.grid_z);
    switch (p.kernel) {
        case GCK_K_TILED:
#define X(CIG, COG, STRIDE, GB, TT, RESID)                                                                                                     \
    if (p.cig == CIG && p.cog == COG && p.stride == STRIDE && p.gb == GB && p.tt == TT && p.resid == RESID)                                    \
        return gconv_launch_planned<gconv_k_kernel<CIG, COG, STRIDE, GB, TT, RESID>>(p, grid, "gconv_general", s, x, wp, bias, alpha, y, c.T_in, \
                                                                                     p.T_out, c.C_in, c.C_out, c.ks);
            GCONV_K_SPECS(X)
#undef X
            break;
        case GCK_K_C1:
            if (p.tt == 32)
                return gconv_launch_planned<gconv_k_c1_kernel<10, 20, 32>>(p, grid, "gconv_general (1 channel per group)", s, x, wp, bias, y, c.T_in, p.T_out,
                                                                           c.C_in, c.C_out, c.ks);
            return gconv_launch_planned<gconv_k_c1_kernel<10, 20, 128>>(p, grid, "gconv_general (1 channel per group)", s, x, wp, bias, y, c.T_in, p.T_out,
                                                                        c.C_in, c.C_out, c.ks);
        case GCK_K_ANY: {
            const int64_t total = (int64_t)c.B * p.T_out * c.C_out;
            if (p.resid)
                return gconv_launch_planned<gconv_k_any_kernel<true>>(p, grid, "gconv_general (any width)", s, x, wp, bias, alpha, y, c.T_in, p.T_out, c.C_in,
                                                                      c.C_out, p.cig, p.cog, p.stride, c.ks, total);
            return gconv_launch_planned<gconv_k_any_kernel<false>>(p, grid, "gconv_general (any width)", s, x, wp, bias, alpha, y, c.T_in, p.T_out, c.C_in,
                                                                   c.C_out, p.cig, p.cog, p.stride, c.ks, total);
        }
        default: break;
    }
    set_error("gconv_general: the plan names a kernel that is not built (family %d, %d -> %d channels per group, stride %d, %d groups x %d steps)",
              p.kernel, p.cig, p.cog, p.stride, p.gb, p.tt);
    return TAL_EINVAL;
}

}  // namespace

int launch_gconv_s2_k(const float* x, const float* wp, const float* bias, int B, int64_t T_in, int C_in, int C_out, int groups,
                      int ks, float* y, hipStream_t s) {
    TAL_CHECK_ARG(x && wp && bias && y, "tal_gconv_s2_k_fwd: null pointer");
    GconvCall c = gconv_call(GE_S2_K, B, T_in, C_in, C_out, groups, ks, x);
    c.has_y = true;
    return launch_planned_k(c, x, wp, bias, 0.f, y, s);
}

int launch_gconv_res_k(const float* x, const float* wp, const float* bias, float alpha, int B, int64_t T, int C, int groups, int ks,
                       float* y, hipStream_t s) {
    TAL_CHECK_ARG(x && wp && bias && y, "tal_gconv_res_k_fwd: null pointer");
    TAL_CHECK_ARG(x != y, "tal_gconv_res_k_fwd: in-place not supported (halo reads)");
    GconvCall c = gconv_call(GE_RES_K, B, T, C, C, groups, ks, x);
    c.has_y = true;
    return launch_planned_k(c, x, wp, bias, alpha, y, s);
}

}  // namespace tal

extern "C" int tal_gconv_s2_k_fwd(const float* x, const float* w_packed, const float* bias, int B, int64_t T_in, int C_in, int C_out,
                                  int groups, int ksize, float* y, void* stream) {
    return tal::launch_gconv_s2_k(x, w_packed, bias, B, T_in, C_in, C_out, groups, ksize, y, (hipStream_t)stream);
}

extern "C" int tal_gconv_res_k_fwd(const float* x, const float* w_packed, const float* bias, float alpha, int B, int64_t T, int C,
                                   int groups, int ksize, float* y, void* stream) {
    return tal::launch_gconv_res_k(x, w_packed, bias, alpha, B, T, C, groups, ksize, y, (hipStream_t)stream);
}
