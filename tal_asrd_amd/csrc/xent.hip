// Teacher-forced scoring without the logits: per row r of a head z[r, s] = feat[r, :] . W[s, :] + b[s]
//   lse[r] = log sum_s exp(z[r, s]),  nll[r] = lse[r] - z[r, target[r]],  top1[r] = arg-max_s z[r, s] (first index among equal values)
// A target is only ever COMPARED with the column index a logit belongs to, never used as an address: target < 0 skips the row's
// loss (nll = 0), target >= N finds no column (nll = +inf).
//
// FUSED FORM (E = 64: the factorised LM head; E = 128: the speaker head): head_stream_kernel<E, XentScan> (csrc/head_stream.h: the
// feature strip in registers, W through LDS, the logits through a wave-private LDS tile, two lanes per row scanning 16 columns
// each, the online log-sum-exp).  The policy keeps the running arg-max and the target's logit, taken when the target's column is
// among the 16 -- the same value the sum saw, so nll >= 0 up to rounding and lse - nll is the logit.
// A workgroup leaves, per row, per slot and per lane half, (max, sum, best value, best index, target logit or -inf = "not seen");
// xent_merge_kernel -- one wave per row, one partial per lane -- adds the sums rescaled to the common maximum in a fixed butterfly
// order, takes the best (value, index) and the one target logit that was seen: bit-identical call after call.
//
// GENERIC FORM (any E the dense layer takes): the logits of a chunk of rows go to the workspace through the dense layer (<= 64 MiB),
// xent_lse_rows_kernel -- one wave per row -- reads them back.  The same kernel is tal_xent_lse_rows.
#include "head_stream.h"

namespace tal {

namespace {

// rows at and above which auto dispatch takes the fused form, per feature width.
// E = 64 (the factorised LM head): the fused form measured faster than the generic one at EVERY row count of the sweep in
// profiles/lm_xent.txt, whose smallest is 64 rows ((D, E0, V) = (512, 64, 16008): generic 0.119 ms, fused 0.098; (256, 64, 10000):
// 0.081 / 0.076; at 16,384 rows 2.249 / 0.506 and 1.064 / 0.320).  Below 64 rows nothing was measured, so nothing is assumed.
// E = 128 (the speaker head): FUSED_FROM_ROWS of csrc/head_topk.hip, the cross-over of the same skeleton at this width
// (profiles/head_topk.txt).  The sweep of THIS kernel (profiles/lm_xent.txt, last table) puts its own cross-over lower -- 256 rows:
// generic 0.060 ms, fused 0.076; 512 rows: 0.073 / 0.064 -- so the constant is on the safe side between 512 and 3,750 rows
// (the generic form there costs up to 0.17 against 0.10 ms at 4,096 rows); lowering it to 512 is a follow-up with its own run.
constexpr int64_t FUSED_FROM_ROWS_E64 = 64, FUSED_FROM_ROWS_E128 = 3751;
inline int64_t fused_from_rows(int E) { return E == 64 ? FUSED_FROM_ROWS_E64 : FUSED_FROM_ROWS_E128; }

// the column a target can match: -1 (no column) for a skipped row and for a target past the head
__device__ __forceinline__ int target_col(int64_t t, int N) { return t >= 0 && t < (int64_t)N ? (int)t : -1; }

// One row per wave, one partial per lane (empty: (-inf, 0), (-inf, NOIDX), -inf): lse from the sums rescaled to the common
// maximum, the best (value, index), the target's logit (at most one lane saw it: the maximum over the lanes is that value).
__device__ __forceinline__ void wave_finish(float mx, float sm, float bv, int bi, float tz, int64_t tgt, int64_t row, int lane,
                                            float* __restrict__ nll, float* __restrict__ lse, int32_t* __restrict__ top1) {
    const float L = lse_lanes(mx, sm);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
        tz = fmaxf(tz, __shfl_xor(tz, off, 64));
    }
    if (lane == 0) {
        // (a target on a -inf column, or on no column at all, has probability 0)
        nll[row] = tgt < 0 ? 0.f : (tz > -INFINITY ? L - tz : INFINITY);
        if (lse) lse[row] = L;
        if (top1) top1[row] = bi;
    }
}

// the fused form's policy: running arg-max and the target's logit; partials [M, HP, 2] x ((max, sum, best value, target logit) | best index)
struct XentScan {
    struct Args {
        const int64_t* target;
        float* part_f;
        int32_t* part_i;
    };
    float bv = -INFINITY, tz = -INFINITY;
    int bi = NOIDX, tcol = -1;
    __device__ __forceinline__ void begin(const Args& a, int64_t row, int64_t M, int S) {
        tcol = row < M ? target_col(a.target[row], S) : -1;
        bv = -INFINITY;
        bi = NOIDX;
        tz = -INFINITY;
    }
    __device__ __forceinline__ void block(const float (&x)[16], int col0, int nv) {
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            if (c < nv && better(x[c], col0 + c, bv, bi)) {
                bv = x[c];
                bi = col0 + c;
            }
            if (col0 + c == tcol) tz = x[c];        // (tcol < S: an existing column)
        }
    }
    __device__ __forceinline__ void leave(const Args& a, int64_t base, const LseState& lse) const {
        f32x4 p = {lse.mx, lse.sm, bv, tz};
        *reinterpret_cast<f32x4*>(a.part_f + base * 4) = p;
        a.part_i[base] = bi;
    }
};

// one wave per row: lane p < 2 x (workgroups on the row's block) takes partial p
__global__ __launch_bounds__(256) void xent_merge_kernel(const float* __restrict__ part_f, const int32_t* __restrict__ part_i,
                                                        const int64_t* __restrict__ target, int64_t M, int NT, int64_t U, int64_t G,
                                                        int HP, float* __restrict__ nll, float* __restrict__ lse,
                                                        int32_t* __restrict__ top1) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int64_t m = row / HS_BM;
    const int P = 2 * (int)(block_of(m * NT + NT - 1, U, G) - block_of(m * NT, U, G) + 1);
    float mx = -INFINITY, sm = 0.f, bv = -INFINITY, tz = -INFINITY;
    int bi = NOIDX;
    if (lane < P) {
        const int64_t base = row * HP * 2 + lane;
        const f32x4 p = *reinterpret_cast<const f32x4*>(part_f + base * 4);
        mx = p.x;
        sm = p.y;
        bv = p.z;
        tz = p.w;
        bi = part_i[base];
    }
    wave_finish(mx, sm, bv, bi, tz, target[row], row, lane, nll, lse, top1);
}

// the rows of a materialised matrix, one wave per row: lane l walks columns l, l + 64, ...
__global__ __launch_bounds__(256) void xent_lse_rows_kernel(const float* __restrict__ x, int64_t M, int N,
                                                           const int64_t* __restrict__ target, float* __restrict__ nll,
                                                           float* __restrict__ lse, int32_t* __restrict__ top1) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* xr = x + row * N;
    const int64_t tgt = target[row];
    const int tcol = target_col(tgt, N);
    float mx = -INFINITY, sm = 0.f, bv = -INFINITY, tz = -INFINITY;
    int bi = NOIDX;
    for (int i = lane; i < N; i += 64) {
        const float v = xr[i];
        if (v > mx) {
            sm = sm * __expf(mx - v) + 1.f;       // (mx == -inf: sm is 0)
            mx = v;
        } else if (mx > -INFINITY) {
            sm += __expf(v - mx);
        }
        if (better(v, i, bv, bi)) {
            bv = v;
            bi = i;
        }
        if (i == tcol) tz = v;
    }
    wave_finish(mx, sm, bv, bi, tz, tgt, row, lane, nll, lse, top1);
}

// two workgroups per CU by default
RunPlan xent_plan(int64_t M, int S) { return head_plan(M, S, HS_BM, HS_BN, HS_SLOTS, 2, device_cus(), opt(OPT_XENT_GRID)); }

// per row, slot and lane half: (max, sum, best value, target logit) and the best index
size_t fused_ws_bytes(int64_t M, int S) { return (size_t)M * xent_plan(M, S).hp * 2 * 20; }

size_t generic_ws_bytes(int64_t M, int S) { return (size_t)generic_chunk_rows(M, S) * (size_t)S * 4; }

bool fused_shape(int E) { return E == 64 || E == 128; }

// the form the dispatch takes BY SHAPE under the options in force (alignment is only known at the call)
bool fused_by_shape(int64_t M, int E) {
    const int form = opt(OPT_XENT_FORM);
    return fused_shape(E) && (form == 2 || (form == 0 && M >= fused_from_rows(E)));
}

// What a call is given: the fused form's partials where the dispatch takes it by shape -- and at least one row of logits, so that
// operands off the 16-byte grid can still run the generic form there, a few rows at a time -- else 64 MiB worth of the generic
// form's logits (which runs on any workspace that holds one row).
size_t xent_rows_ws_bytes(int64_t M, int N, int E) {
    if (!fused_by_shape(M, E)) return generic_ws_bytes(M, N);
    const size_t fused = fused_ws_bytes(M, N), row = (size_t)N * 4;
    return fused > row ? fused : row;
}

int launch_xent_lse_rows(const float* x, int64_t M, int N, const int64_t* target, float* nll, float* lse, int32_t* top1, hipStream_t s) {
    ProfScope prof(PROF_OTHER, (double)M * N * 4.0, s);
    hipLaunchKernelGGL(xent_lse_rows_kernel, dim3((unsigned)cdiv(M, 4)), dim3(256), 0, s, x, M, N, target, nll, lse, top1);
    TAL_CHECK_LAUNCH("xent_lse_rows");
    return TAL_OK;
}

int launch_xent_fused(const float* feat, int64_t ldf, int E, const float* w, const float* b, const int64_t* target, int64_t M, int S,
                      float* nll, float* lse, int32_t* top1, void* workspace, hipStream_t s) {
    const int NT = (int)cdiv(S, HS_BN);
    const int64_t U = cdiv(M, HS_BM) * NT;
    const RunPlan plan = xent_plan(M, S);
    const int64_t grid = plan.grid;
    const int hp = plan.hp;
    float* pf = reinterpret_cast<float*>(workspace);
    int32_t* pi = reinterpret_cast<int32_t*>(pf + (size_t)M * hp * 2 * 4);
    {
        ProfScope prof(PROF_GEMM, 2.0 * (double)M * (double)S * E, s);
        const XentScan::Args args = {target, pf, pi};
        if (E == 64)
            hipLaunchKernelGGL((head_stream_kernel<64, XentScan>), dim3((unsigned)grid), dim3(256), 0, s, feat, ldf, w, b, M, S, NT, U, args, hp);
        else
            hipLaunchKernelGGL((head_stream_kernel<128, XentScan>), dim3((unsigned)grid), dim3(256), 0, s, feat, ldf, w, b, M, S, NT, U, args, hp);
        TAL_CHECK_LAUNCH("xent");
    }
    ProfScope prof(PROF_OTHER, (double)M * hp * 2 * 20.0, s);
    hipLaunchKernelGGL(xent_merge_kernel, dim3((unsigned)cdiv(M, 4)), dim3(256), 0, s, pf, pi, target, M, NT, U, grid, hp, nll, lse, top1);
    TAL_CHECK_LAUNCH("xent(merge)");
    return TAL_OK;
}

bool fused_possible(const float* feat, int64_t ldf, const float* w, int E) {
    return fused_shape(E) && ldf % 4 == 0 && ((reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(w)) & 15) == 0;
}

// tal_xent_rows_fwd behind its argument checks (tal_lm_xent_fwd calls it on the projected rows)
int xent_rows(const char* who, const float* feat, int64_t M, int64_t ldf, int E, const float* w, const float* bias, int N,
              const int64_t* target, float* nll, float* lse, int32_t* top1, void* workspace, size_t workspace_bytes, hipStream_t s) {
    const int form = opt(OPT_XENT_FORM);
    TAL_CHECK_ARG(form != 2 || fused_possible(feat, ldf, w, E),
                  "%s: the fused form needs E == 64 or 128, a row pitch that is a multiple of 4 and 16-byte aligned operands (E=%d)", who, E);
    const bool fused = fused_by_shape(M, E) && fused_possible(feat, ldf, w, E);
    const size_t need = fused ? fused_ws_bytes(M, N) : (size_t)N * 4;        // (generic: one row of logits at least)
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace %zu < %zu bytes", who, workspace ? workspace_bytes : (size_t)0, need);
        return TAL_ENOMEM;
    }
    TAL_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
    if (fused) return launch_xent_fused(feat, ldf, E, w, bias, target, M, N, nll, lse, top1, workspace, s);
    // the logits of a chunk of rows through the dense layer (launch_linear's launch, with the features' row pitch), then the row kernel
    // (as many rows at a time as the workspace holds, 64 MiB worth at most: tal_xent_rows_workspace_bytes asks for that much where
    //  it expects this form; a smaller workspace means more, shorter launches)
    int64_t chunk = generic_chunk_rows(M, N);
    const int64_t fit = (int64_t)(workspace_bytes / ((size_t)N * 4));
    chunk = fit < chunk ? fit : chunk;
    float* logits = reinterpret_cast<float*>(workspace);
    for (int64_t r0 = 0; r0 < M; r0 += chunk) {
        const int64_t rows = M - r0 < chunk ? M - r0 : chunk;
        int rc = ldf == E ? launch_linear(feat + r0 * ldf, w, bias, nullptr, 0.f, 0, rows, N, E, logits, s)
                          : launch_linear_ld(feat + r0 * ldf, ldf, w, bias, rows, N, E, logits, N, s);
        if (rc) return rc;
        rc = launch_xent_lse_rows(logits, rows, N, target + r0, nll + r0, lse ? lse + r0 : nullptr, top1 ? top1 + r0 : nullptr, s);
        if (rc) return rc;
    }
    return TAL_OK;
}

}  // namespace

}  // namespace tal

using namespace tal;

extern "C" size_t tal_xent_rows_workspace_bytes(int64_t M, int N, int E) {
    if (M <= 0 || N <= 0 || E <= 0) return 0;
    return xent_rows_ws_bytes(M, N, E);
}

extern "C" int tal_xent_rows_fwd(const float* feat, int64_t M, int64_t ldf, int E, const float* w, const float* bias, int N,
                                 const int64_t* target, float* nll, float* lse, int32_t* top1, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    TAL_CHECK_ARG(M >= 0 && E > 0 && N > 0 && ldf >= E, "tal_xent_rows_fwd: bad shape (M=%lld, ldf=%lld, E=%d, N=%d)", (long long)M,
                  (long long)ldf, E, N);
    if (M == 0) return TAL_OK;
    TAL_CHECK_ARG(feat && w && target && nll, "tal_xent_rows_fwd: null pointer");
    return xent_rows("tal_xent_rows_fwd", feat, M, ldf, E, w, bias, N, target, nll, lse, top1, workspace, workspace_bytes,
                     (hipStream_t)stream);
}

extern "C" int tal_xent_lse_rows(const float* x, int64_t M, int N, const int64_t* target, float* nll, float* lse, int32_t* top1,
                                 void* stream) {
    TAL_CHECK_ARG(M >= 0 && N > 0, "tal_xent_lse_rows: bad shape (M=%lld, N=%d)", (long long)M, N);
    if (M == 0) return TAL_OK;
    TAL_CHECK_ARG(x && target && nll, "tal_xent_lse_rows: null pointer");
    return launch_xent_lse_rows(x, M, N, target, nll, lse, top1, (hipStream_t)stream);
}

extern "C" size_t tal_lm_xent_workspace_bytes(int64_t M, int D, int E0, int V) {
    if (M <= 0 || D <= 0 || E0 <= 0 || V <= 0) return 0;
    return lm_proj_bytes(M, E0) + xent_rows_ws_bytes(M, V, E0);
}

extern "C" int tal_lm_xent_fwd(const float* h, int64_t M, int64_t ldh, int D, const float* proj_t, int E0, const float* emb, int V,
                               const int64_t* target, float* nll, float* lse, int32_t* top1, void* workspace, size_t workspace_bytes,
                               void* stream) {
    TAL_CHECK_ARG(M >= 0 && D > 0 && E0 > 0 && V > 0 && ldh >= D && ldh % 4 == 0, "tal_lm_xent_fwd: bad shape");
    TAL_CHECK_ARG(proj_t || D == E0, "tal_lm_xent_fwd: no projection needs D == E0");
    if (M == 0) return TAL_OK;
    TAL_CHECK_ARG(h && emb && target && nll, "tal_lm_xent_fwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (!proj_t)
        return xent_rows("tal_lm_xent_fwd", h, M, ldh, D, emb, nullptr, V, target, nll, lse, top1, workspace, workspace_bytes, s);
    return lm_head_project(
        "tal_lm_xent_fwd", h, M, ldh, D, proj_t, E0, workspace, workspace_bytes, s,
        [&](const float* t, size_t& need) -> int {
            TAL_CHECK_ARG(opt(OPT_XENT_FORM) != 2 || fused_possible(t, E0, emb, E0),
                          "tal_lm_xent_fwd: the fused form needs E0 == 64 or 128 and 16-byte aligned operands (E0=%d)", E0);
            need = fused_by_shape(M, E0) && fused_possible(t, E0, emb, E0) ? fused_ws_bytes(M, V) : (size_t)V * 4;
            return TAL_OK;
        },
        [&](const float* t, void* ws, size_t ws_bytes) {
            return xent_rows("tal_lm_xent_fwd", t, M, E0, E0, emb, nullptr, V, target, nll, lse, top1, ws, ws_bytes, s);
        });
}
