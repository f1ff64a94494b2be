// Waveform resampling on the device: torchaudio 0.4.0's kaldi.resample_waveform (what the reference's loaders run on the CPU after
// torchaudio.load, tal/asr/data/util.py:45-48), restated.  For integer rates orig -> new and lowpass_filter_width `width`:
//   g = gcd(orig, new), iu = orig / g input samples and ou = new / g outputs ("phases") per unit;
//   fc = 0.99 * 0.5 * min(orig, new), ww = width / (2 fc);  phase p: t_p = p / new,
//   first[p] = ceil((t_p - ww) orig), last[p] = floor((t_p + ww) orig), taps = max_p (last[p] - first[p] + 1);
//   w[p][j] at dt = (first[p] + j) / orig - t_p:  0 where |dt| >= ww, else 0.5 (1 + cos(2 pi fc / width dt)) sinc / orig with
//   sinc = sin(2 pi fc dt) / (pi dt), 2 fc at dt = 0;
//   y[q ou + p] = sum_j w[p][j] x[q iu + first[p] + j], x = 0 outside [0, L);  n_out(L) = ceil(L ou / iu).
// The table is computed once on the host in double and rounded to fp32 (rs_build: the one place the formula lives).
//
// Kernel: a workgroup of 256 lanes walks tiles of `tm` consecutive outputs of one item (grid-stride over item x tile).  The input
// index q iu + first[p] never decreases with the output index, so a tile reads ONE contiguous span of the input: it is staged
// into LDS as fp32 with 16-byte loads (the span start is moved back to the 16-byte boundary below it, whatever the element
// type and offset; vectors that touch the outside of [0, length) go element by element with the zero fill), int16 samples
// scaled by 2^-15 and fp16 samples widened, both exactly.  Lane t then produces outputs t, t + 256, ... of the tile: consecutive
// lanes are on consecutive phases, the phase rows sit in LDS at an ODD stride (no two of 32 consecutive rows share a bank),
// and every output is one fp32 FMA chain over j = 0 .. taps - 1 in that order -- a function of (p, the taps samples) alone, so
// results do not depend on tiling, batch position or timing.  Rate pairs whose table does not fit beside the slab (16001 ->
// 16000: 16000 phases) run the same kernel with the rows read from global memory (L2-resident: the table is at most 4 MiB).
// All sample indices are 64-bit; tile-local ones (below the slab size) are 32-bit.
#include <math.h>

#include <cstring>
#include <vector>

#include "common.h"

namespace tal {

constexpr int RS_MAGIC = 0x52534d31;              // plan header word 0
constexpr int RS_RATE_MAX = 1 << 20;              // largest sample rate (Hz) on either side
constexpr int RS_WIDTH_MAX = 64;                  // largest lowpass_filter_width
constexpr int RS_TAPS_MAX = 1024;                 // longest filter (orig / new up to ~80 at width 6)
constexpr int64_t RS_TABLE_MAX = (int64_t)1 << 20;    // most table entries (phases x taps) a plan holds
constexpr int RS_SLAB = 6144;                     // floats of staged input per tile (24 KiB)
constexpr int RS_TABLE_LDS = 10240;               // floats of table (rows at the odd stride + first[]) kept in LDS (40 KiB)
constexpr int RS_TM_MAX = 4096, RS_TM_MIN = 64;   // outputs per tile
constexpr size_t RS_HDR = 256;                    // plan: header, first[ou] at RS_HDR, w[ou][taps] at rs_woff(ou)

__host__ __device__ inline size_t rs_woff(int ou) { return (RS_HDR + (size_t)ou * 4 + 255) & ~(size_t)255; }

// n_out(L) = number of output instants m / new < L / orig, i.e. m iu < L ou
__host__ __device__ inline int64_t rs_num_samples(int64_t L, int iu, int ou) {
    if (L <= 0) return 0;
    const int64_t t = L * ou;
    int64_t last = t / iu;
    if (last * iu == t) --last;
    return last + 1;
}

struct RShape {
    int iu, ou, taps, tm, S;
    bool lds;        // the table fits in LDS
};

static int rs_gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

#pragma clang fp contract(off)
static void rs_phase(int p, int orig, int nw, int width, int* first, int* last) {
    const double fc = 0.99 * 0.5 * (double)(orig < nw ? orig : nw);
    const double ww = (double)width / (2.0 * fc);
    const double tp = (double)p / (double)nw;
    *first = (int)ceil((tp - ww) * (double)orig);
    *last = (int)floor((tp + ww) * (double)orig);
}

// -> NULL and the shape, or the violated limit
static const char* rs_shape(int orig, int nw, int width, RShape* out) {
    static thread_local int c_orig = 0, c_new = 0, c_width = 0;    // (the shape of the last pair asked for: the loop below walks
    static thread_local RShape c_shape;                            //  every phase, 16000 of them for 16001 -> 16000)
    if (orig < 1 || orig > RS_RATE_MAX || nw < 1 || nw > RS_RATE_MAX) return "sample rates must be 1..1048576 Hz";
    if (width < 1 || width > RS_WIDTH_MAX) return "lowpass_filter_width must be 1..64";
    if (orig == c_orig && nw == c_new && width == c_width) {
        *out = c_shape;
        return NULL;
    }
    RShape s;
    const int g = rs_gcd(orig, nw);
    s.iu = orig / g;
    s.ou = nw / g;
    s.taps = 0;
    int prev = 0, f0 = 0;
    for (int p = 0; p < s.ou; ++p) {
        int f, l;
        rs_phase(p, orig, nw, width, &f, &l);
        if (l - f + 1 > s.taps) s.taps = l - f + 1;
        if (p == 0) f0 = f;
        else if (f < prev) return "internal: first[] decreases";     // (the kernel's one-span staging rests on this order)
        prev = f;
    }
    if (f0 + s.iu < prev) return "internal: first[] decreases across the unit";
    if (s.taps < 1 || s.taps > RS_TAPS_MAX) return "the filter is longer than 1024 taps (orig / new too large)";
    if ((int64_t)s.ou * s.taps > RS_TABLE_MAX) return "the table (phases x taps = new / gcd x taps) exceeds 2^20 entries";
    s.S = s.taps | 1;
    s.lds = (int64_t)s.ou * (s.S + 1) <= RS_TABLE_LDS;
    // outputs per tile: their input span, ceil(tm orig / new) + taps + 2, plus the alignment slack of 16 elements, fits the slab
    int64_t tm = (int64_t)(RS_SLAB - s.taps - 18) * nw / orig;
    tm = tm > RS_TM_MAX ? RS_TM_MAX : tm / 64 * 64;
    if (tm < RS_TM_MIN) return "a tile of 64 outputs does not fit the staging buffer (orig / new too large)";
    s.tm = (int)tm;
    c_orig = orig;
    c_new = nw;
    c_width = width;
    c_shape = s;
    *out = s;
    return NULL;
}

// the table in double, rounded to fp32: w [ou][taps] (may be NULL), first [ou] (may be NULL)
static void rs_build(int orig, int nw, int width, const RShape& s, float* w, int32_t* first) {
    const double pi = 3.14159265358979323846264338327950288;
    const double fc = 0.99 * 0.5 * (double)(orig < nw ? orig : nw);
    const double ww = (double)width / (2.0 * fc);
    for (int p = 0; p < s.ou; ++p) {
        int f, l;
        rs_phase(p, orig, nw, width, &f, &l);
        if (first) first[p] = f;
        if (!w) continue;
        const double tp = (double)p / (double)nw;
        for (int j = 0; j < s.taps; ++j) {
            const double dt = (double)(f + j) / (double)orig - tp;
            double v = 0.0;
            if (fabs(dt) < ww) {
                const double win = 0.5 * (1.0 + cos(2.0 * pi * fc / (double)width * dt));
                const double sinc = dt == 0.0 ? 2.0 * fc : sin(2.0 * pi * fc * dt) / (pi * dt);
                v = win * sinc / (double)orig;
            }
            w[(size_t)p * s.taps + j] = (float)v;
        }
    }
}

struct RArgs {
    const char* plan;
    const void* x;
    const int64_t* lengths;
    float* y;
    int64_t L, N, x_pitch, y_pitch, nt, total;
    int orig, nw, width, iu, ou, taps, tm, S;
};

template <typename XT>
struct RsIn;
template <>
struct RsIn<float> {
    static constexpr int V = 4;
    typedef f32x4 vec;
    static __device__ __forceinline__ float cvt(float v) { return v; }
};
template <>
struct RsIn<_Float16> {
    static constexpr int V = 8;
    typedef f16x8 vec;
    static __device__ __forceinline__ float cvt(_Float16 v) { return (float)v; }
};
template <>
struct RsIn<int16_t> {
    static constexpr int V = 8;
    typedef short vec __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ float cvt(short v) { return (float)v * 0x1p-15f; }     // exact: |v| <= 2^15
};

template <typename XT, bool TLDS>
__global__ __launch_bounds__(256) void resample_kernel(RArgs a) {
    typedef RsIn<XT> In;
    constexpr int V = In::V;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* slab = lds;
    int* lfirst = reinterpret_cast<int*>(lds + RS_SLAB);
    float* lw = lds + RS_SLAB + a.ou;
    const int tid = threadIdx.x;
    const int ou = a.ou, iu = a.iu, taps = a.taps;
    const int* hdr = reinterpret_cast<const int*>(a.plan);
    const int* gfirst = reinterpret_cast<const int*>(a.plan + RS_HDR);
    const float* gw = reinterpret_cast<const float*>(a.plan + rs_woff(ou));
    // a plan built for another rate pair: every output of this call (the caller's shape, in bounds) becomes NaN
    const bool bad = hdr[0] != RS_MAGIC || hdr[1] != a.orig || hdr[2] != a.nw || hdr[3] != a.width || hdr[4] != taps;
    if (TLDS && !bad) {
        for (int p = tid; p < ou; p += 256) lfirst[p] = gfirst[p];
        for (int i = tid; i < ou * taps; i += 256) {
            const int p = i / taps;
            lw[p * a.S + (i - p * taps)] = gw[i];
        }
        __syncthreads();
    }
    const int* first = TLDS ? lfirst : gfirst;
    const int stq = 256 / ou, stp = 256 - stq * ou;
    for (int64_t tile = blockIdx.x; tile < a.total; tile += gridDim.x) {
        const int64_t b = tile / a.nt;
        const int64_t m0 = (tile - b * a.nt) * a.tm;
        const int cnt = (int)(a.N - m0 < a.tm ? a.N - m0 : a.tm);
        float* yb = a.y + b * a.y_pitch + m0;
        int64_t lim = a.L;
        if (a.lengths) {
            const int64_t l = a.lengths[b];
            lim = l < 0 ? 0 : (l < lim ? l : lim);
        }
        const int64_t nout = rs_num_samples(lim, iu, ou);
        const int64_t q0 = m0 / ou, q1 = (m0 + cnt - 1) / ou;
        const int p0 = (int)(m0 - q0 * ou), p1 = (int)(m0 + cnt - 1 - q1 * ou);
        const int first0 = bad ? 0 : first[p0];
        const int64_t s0 = q0 * iu + first0;
        const int64_t s1 = bad ? s0 : q1 * iu + first[p1] + taps;        // one past the last sample the tile reads
        const XT* xb = reinterpret_cast<const XT*>(a.x) + b * a.x_pitch;
        const uintptr_t addr = reinterpret_cast<uintptr_t>(xb) + (uintptr_t)(s0 * (int64_t)sizeof(XT));
        const int lead = (int)((addr & 15) / sizeof(XT));                // elements back to the 16-byte boundary
        const int64_t sb = s0 - lead;
        const int nvec = (int)((s1 - sb + V - 1) / V);
        if (bad || m0 >= nout || nvec * V > RS_SLAB) {                   // (block-uniform; the last never holds: rs_shape sized tm)
            const float fill = m0 >= nout && !bad ? 0.f : __builtin_nanf("");
            for (int o = tid; o < cnt; o += 256) yb[o] = fill;
            continue;
        }
        __syncthreads();             // the previous tile's readers are done with the slab
        for (int k = tid; k < nvec; k += 256) {
            const int64_t e = sb + (int64_t)k * V;
            float* d = slab + k * V;
            if (e >= 0 && e + V <= lim) {
                const typename In::vec v = *reinterpret_cast<const typename In::vec*>(xb + e);
#pragma unroll
                for (int i = 0; i < V; i += 4) {
                    const f32x4 f = {In::cvt(v[i]), In::cvt(v[i + 1]), In::cvt(v[i + 2]), In::cvt(v[i + 3])};
                    *reinterpret_cast<f32x4*>(d + i) = f;
                }
            } else {
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const int64_t ee = e + i;
                    d[i] = (ee >= 0 && ee < lim) ? In::cvt(xb[ee]) : 0.f;
                }
            }
        }
        __syncthreads();
        int dq = (p0 + tid) / ou;
        int p = p0 + tid - dq * ou;
        for (int o = tid; o < cnt; o += 256) {
            const float* xs = slab + (dq * iu + (first[p] - first0) + lead);
            const float* wr = TLDS ? lw + p * a.S : gw + (size_t)p * taps;
            float acc = 0.f;
            for (int j = 0; j < taps; ++j) acc = fmaf(wr[j], xs[j], acc);
            yb[o] = m0 + o < nout ? acc : 0.f;
            p += stp;
            dq += stq;
            if (p >= ou) {
                p -= ou;
                ++dq;
            }
        }
    }
}

template <typename XT>
static int rs_launch(const RArgs& a, const RShape& sh, hipStream_t s) {
    const size_t lds = ((size_t)RS_SLAB + (sh.lds ? (size_t)sh.ou * (sh.S + 1) : 0)) * sizeof(float);     // <= 64 KiB
    int per_cu = (int)((size_t)160 * 1024 / lds);
    per_cu = per_cu > 8 ? 8 : per_cu;
    const int64_t cap = (int64_t)device_cus() * per_cu;
    const unsigned grid = (unsigned)(a.total < cap ? a.total : cap);
    if (sh.lds)
        hipLaunchKernelGGL((resample_kernel<XT, true>), dim3(grid), dim3(256), lds, s, a);
    else
        hipLaunchKernelGGL((resample_kernel<XT, false>), dim3(grid), dim3(256), lds, s, a);
    TAL_CHECK_LAUNCH("tal_resample_fwd");
    return TAL_OK;
}

}  // namespace tal

using namespace tal;

extern "C" int64_t tal_resample_num_samples(int64_t n_in, int orig, int new_rate) {
    if (orig < 1 || new_rate < 1 || n_in <= 0) return 0;
    const int g = rs_gcd(orig, new_rate);
    return rs_num_samples(n_in, orig / g, new_rate / g);
}

extern "C" size_t tal_resample_plan_bytes(int orig, int new_rate, int width) {
    RShape sh;
    if (rs_shape(orig, new_rate, width, &sh)) return 0;
    return rs_woff(sh.ou) + (((size_t)sh.ou * sh.taps * 4 + 255) & ~(size_t)255);
}

extern "C" int tal_resample_plan_build_host(int orig, int new_rate, int width, float* w, int32_t* first, int* taps) {
    RShape sh;
    const char* err = rs_shape(orig, new_rate, width, &sh);
    TAL_CHECK_ARG(!err, "tal_resample_plan_build_host(%d -> %d, width %d): %s", orig, new_rate, width, err);
    if (taps) *taps = sh.taps;
    rs_build(orig, new_rate, width, sh, w, first);
    return TAL_OK;
}

extern "C" int tal_resample_plan_init(void* plan, int orig, int new_rate, int width, void* stream) {
    TAL_CHECK_ARG(plan, "tal_resample_plan_init: null pointer");
    RShape sh;
    const char* err = rs_shape(orig, new_rate, width, &sh);
    TAL_CHECK_ARG(!err, "tal_resample_plan_init(%d -> %d, width %d): %s", orig, new_rate, width, err);
    const size_t bytes = tal_resample_plan_bytes(orig, new_rate, width);
    std::vector<char> buf(bytes, 0);
    const int hdr[8] = {RS_MAGIC, orig, new_rate, width, sh.taps, sh.iu, sh.ou, sh.tm};
    memcpy(buf.data(), hdr, sizeof(hdr));
    rs_build(orig, new_rate, width, sh, reinterpret_cast<float*>(buf.data() + rs_woff(sh.ou)),
             reinterpret_cast<int32_t*>(buf.data() + RS_HDR));
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(plan, buf.data(), bytes, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        set_error("tal_resample_plan_init: cannot upload the plan");
        return TAL_EHIP;
    }
    return TAL_OK;
}

extern "C" int tal_resample_fwd(const void* plan, int orig, int new_rate, int width, const void* x, int x_dtype, int B, int64_t L_in,
                                int64_t x_pitch, const int64_t* lengths, float* y, int64_t y_pitch, void* stream) {
    const char* what = "tal_resample_fwd";
    RShape sh;
    const char* err = rs_shape(orig, new_rate, width, &sh);
    TAL_CHECK_ARG(!err, "%s(%d -> %d, width %d): %s", what, orig, new_rate, width, err);
    TAL_CHECK_ARG(x_dtype == TAL_RESAMPLE_F32 || x_dtype == TAL_RESAMPLE_F16 || x_dtype == TAL_RESAMPLE_I16,
                  "%s: x_dtype=%d is none of fp32 (0), fp16 (1), int16 (2)", what, x_dtype);
    TAL_CHECK_ARG(B > 0 && L_in >= 0, "%s: need B > 0 and L_in >= 0 (B=%d, L_in=%lld)", what, B, (long long)L_in);
    const int64_t N = rs_num_samples(L_in, sh.iu, sh.ou);
    if (N == 0) return TAL_OK;
    TAL_CHECK_ARG(plan && x && y, "%s: null pointer", what);
    const int esz = x_dtype == TAL_RESAMPLE_F32 ? 4 : 2;
    TAL_CHECK_ARG(reinterpret_cast<uintptr_t>(x) % esz == 0 && reinterpret_cast<uintptr_t>(y) % 4 == 0,
                  "%s: x / y must be aligned to their element size", what);
    TAL_CHECK_ARG(x_pitch >= L_in && y_pitch >= N, "%s: pitches (%lld, %lld) below the row lengths (%lld, %lld)", what,
                  (long long)x_pitch, (long long)y_pitch, (long long)L_in, (long long)N);
    RArgs a;
    a.plan = reinterpret_cast<const char*>(plan);
    a.x = x;
    a.lengths = lengths;
    a.y = y;
    a.L = L_in;
    a.N = N;
    a.x_pitch = x_pitch;
    a.y_pitch = y_pitch;
    a.nt = cdiv(N, sh.tm);
    a.total = a.nt * B;
    a.orig = orig;
    a.nw = new_rate;
    a.width = width;
    a.iu = sh.iu;
    a.ou = sh.ou;
    a.taps = sh.taps;
    a.tm = sh.tm;
    a.S = sh.S;
    TAL_CHECK_ARG(a.total < (int64_t)1 << 31, "%s: %lld outputs x %d items is too many tiles", what, (long long)N, B);
    hipStream_t s = (hipStream_t)stream;
    // algorithmic HBM bytes: read L_in samples, write N floats per item
    ProfScope prof(PROF_OTHER, (double)B * ((double)L_in * esz + (double)N * 4.0), s);
    if (x_dtype == TAL_RESAMPLE_F32) return rs_launch<float>(a, sh, s);
    if (x_dtype == TAL_RESAMPLE_F16) return rs_launch<_Float16>(a, sh, s);
    return rs_launch<int16_t>(a, sh, s);
}
