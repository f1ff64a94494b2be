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

int launch_xent_lse_rows(const float* x, int64_t M, int N, const int64_t* target, float* nll, float* lse, int32_t* top1, hipStream_t s) {
    ProfScope prof(PROF_OTHER, (double)M * N * 4.0, s);
    hipLaunchKernelGGL(xent_lse_rows_kernel, dim3((unsigned)cdiv(M, 4)), dim3(256), 0, s, x, M, N, target, nll, lse, top1);
    TAL_CHECK_LAUNCH("xent_lse_rows");
    return TAL_OK;
}

// the fused launch the plan describes
int launch_xent_fused(const HeadLaunch& p, const float* feat, int64_t ldf, int E, const float* w, const float* b, const int64_t* target,
                      int64_t M, int S, float* nll, float* lse, int32_t* top1, void* workspace, hipStream_t s) {
    const int NT = p.NT, hp = p.run.hp;
    const int64_t U = p.U, grid = p.run.grid;
    float* pf = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + p.off[0]);
    int32_t* pi = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(workspace) + p.off[1]);
    {
        ProfScope prof(PROF_GEMM, 2.0 * (double)M * (double)S * E, s);
        const XentScan::Args args = {target, pf, pi};
        if (E == 64)
            hipLaunchKernelGGL((head_stream_kernel<64, XentScan>), dim3((unsigned)grid), dim3(256), 0, s, feat, ldf, w, b, M, S, NT, U, args, hp);
        else
            hipLaunchKernelGGL((head_stream_kernel<128, XentScan>), dim3((unsigned)grid), dim3(256), 0, s, feat, ldf, w, b, M, S, NT, U, args, hp);
        TAL_CHECK_LAUNCH("xent");
    }
    ProfScope prof(PROF_OTHER, (double)p.need, s);
    hipLaunchKernelGGL(xent_merge_kernel, dim3((unsigned)cdiv(M, 4)), dim3(256), 0, s, pf, pi, target, M, NT, U, grid, hp, nll, lse, top1);
    TAL_CHECK_LAUNCH("xent(merge)");
    return TAL_OK;
}

// tal_xent_rows_fwd and tal_lm_xent_fwd behind their argument checks: the head on the rows of h, or on their projection (proj_t != NULL).
// The planned call: the fused launch, or the logits of a chunk of rows through the dense layer (launch_linear's launch, with the
// features' row pitch), then the row kernel (as many rows at a time as the workspace holds, 64 MiB worth at most:
// tal_xent_rows_workspace_bytes asks for that much where it expects this form; a smaller workspace means more, shorter launches)
int xent_rows(int entry, const float* h, int64_t M, int64_t ldh, int D, const float* proj_t, int E0, const float* w, const float* bias, int N,
              const int64_t* target, float* nll, float* lse, int32_t* top1, void* workspace, size_t workspace_bytes, hipStream_t s) {
    return head_on_rows(
        entry, h, M, ldh, D, proj_t, E0, workspace, workspace_bytes, s,
        [&](const float* feat, int64_t ldf, int E, int proj_in, const void* ws, size_t ws_bytes) {
            return head_call(entry, M, N, E, E, 1, ldf, proj_in, feat, w, w, ws, ws_bytes);
        },
        [&](const HeadCall& c, const HeadLaunch& p, const float* feat, void* ws) {
            if (p.fused) return launch_xent_fused(p, feat, c.ldf, c.E, w, bias, target, M, N, nll, lse, top1, ws, s);
            float* logits = reinterpret_cast<float*>(ws);
            return for_row_chunks(M, p.chunk, [&](int64_t r0, int64_t rows) {
                const int rc = c.ldf == c.E ? launch_linear(feat + r0 * c.ldf, w, bias, nullptr, 0.f, 0, rows, N, c.E, logits, s)
                                            : launch_linear_ld(feat + r0 * c.ldf, c.ldf, w, bias, rows, N, c.E, logits, N, s);
                return rc ? rc : launch_xent_lse_rows(logits, rows, N, target + r0, nll + r0, lse ? lse + r0 : nullptr, top1 ? top1 + r0 : nullptr, s);
            });
        });
}

}  // namespace

}  // namespace tal

using namespace tal;

extern "C" size_t tal_xent_rows_workspace_bytes(int64_t M, int N, int E) { return head_query_bytes(head_call(HE_XENT_ROWS, M, N, E, E, 1, E)); }

extern "C" int tal_xent_rows_fwd(const float* feat, int64_t M, int64_t ldf, int E, const float* w, const float* bias, int N,
                                 const int64_t* target, float* nll, float* lse, int32_t* top1, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    TAL_CHECK_ARG(M >= 0 && E > 0 && N > 0 && ldf >= E, "tal_xent_rows_fwd: bad shape (M=%lld, ldf=%lld, E=%d, N=%d)", (long long)M,
                  (long long)ldf, E, N);
    if (M == 0) return TAL_OK;
    TAL_CHECK_ARG(feat && w && target && nll, "tal_xent_rows_fwd: null pointer");
    return xent_rows(HE_XENT_ROWS, feat, M, ldf, E, nullptr, 0, w, bias, N, target, nll, lse, top1, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int tal_xent_lse_rows(const float* x, int64_t M, int N, const int64_t* target, float* nll, float* lse, int32_t* top1,
                                 void* stream) {
    TAL_CHECK_ARG(M >= 0 && N > 0, "tal_xent_lse_rows: bad shape (M=%lld, N=%d)", (long long)M, N);
    if (M == 0) return TAL_OK;
    TAL_CHECK_ARG(x && target && nll, "tal_xent_lse_rows: null pointer");
    return launch_xent_lse_rows(x, M, N, target, nll, lse, top1, (hipStream_t)stream);
}

extern "C" size_t tal_lm_xent_workspace_bytes(int64_t M, int D, int E0, int V) {
    if (D <= 0) return 0;
    const size_t head = head_query_bytes(head_call(HE_LM_XENT, M, V, E0, E0, 1, E0));
    return head ? lm_proj_bytes(M, E0) + head : 0;
}

extern "C" int tal_lm_xent_fwd(const float* h, int64_t M, int64_t ldh, int D, const float* proj_t, int E0, const float* emb, int V,
                               const int64_t* target, float* nll, float* lse, int32_t* top1, void* workspace, size_t workspace_bytes,
                               void* stream) {
    TAL_CHECK_ARG(M >= 0 && D > 0 && E0 > 0 && V > 0 && ldh >= D && ldh % 4 == 0, "tal_lm_xent_fwd: bad shape");
    TAL_CHECK_ARG(proj_t || D == E0, "tal_lm_xent_fwd: no projection needs D == E0");
    if (M == 0) return TAL_OK;
    TAL_CHECK_ARG(h && emb && target && nll, "tal_lm_xent_fwd: null pointer");
    return xent_rows(HE_LM_XENT, h, M, ldh, D, proj_t, E0, emb, nullptr, V, target, nll, lse, top1, workspace, workspace_bytes, (hipStream_t)stream);
}
