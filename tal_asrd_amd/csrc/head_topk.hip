// Per-frame top-k speaker posteriors of the diarization head without the logits:
//   z[r, s] = feat[r, :] . W[s, :] + b[s],  lse[r] = log sum_s exp(z[r, s]),
//   ids[r, 0..k) = the k largest z[r, :] (value descending, index ascending among equal values),  logp[r, j] = z[r, ids[r, j]] - lse[r]
//
// FUSED FORM (E = 128): head_stream_kernel<128, TopkScan<K>> (csrc/head_stream.h: the feature strip in registers, W through LDS,
// the logits through a wave-private LDS tile, two lanes per row scanning 16 columns each, the online log-sum-exp).  The policy keeps
// a sorted list of K (value, index) pairs per lane and compares a logit against the K-th entry first (an insert is rare after the
// first tiles): 2 K registers.  A workgroup leaves, per row, per slot and per lane half, K pairs and (max, sum);
// head_topk_merge_kernel -- one wave per row, one list per lane -- pops the k winners in order and adds the sums, rescaled to the
// common maximum, in a fixed butterfly order: bit-identical call after call.
//
// GENERIC FORM (any E the dense layer takes): the logits of a chunk of rows go to the workspace through launch_linear (<= 64 MiB),
// topk_lse_rows_kernel -- one wave per row -- reads them back.  The same kernel is tal_topk_lse_rows.
#include "head_stream.h"

namespace tal {

namespace {

// (TV / TI: K floats / ints under [], an array or a vector)
template <int K, class TV, class TI>
__device__ __forceinline__ void topk_clear(TV& tv, TI& ti) {
#pragma unroll
    for (int q = 0; q < K; ++q) {
        tv[q] = -INFINITY;
        ti[q] = NOIDX;
    }
}

// insert into the sorted list: the newcomer takes the first place it is better than, everything behind moves down one
template <int K, class TV, class TI>
__device__ __forceinline__ void topk_insert(TV& tv, TI& ti, float v, int i) {
#pragma unroll
    for (int q = 0; q < K; ++q) {
        const bool b = better(v, i, tv[q], ti[q]);
        const float ov = tv[q];
        const int oi = ti[q];
        tv[q] = b ? v : ov;
        ti[q] = b ? i : oi;
        v = b ? ov : v;
        i = b ? oi : i;
    }
}

// One row per wave, one sorted list and one (max, sum) per lane (empty lists: all (-inf, NOIDX), (-inf, 0)): lse from the sums
// rescaled to the common maximum, then k rounds of "best head of all lists wins and is popped".  Column indices are unique across
// the lists, so the winner's lane is the one whose head carries the winning index.
template <int K>
__device__ __forceinline__ void wave_finish(float (&tv)[K], int (&ti)[K], float mx, float sm, int k, int64_t row, int lane,
                                            int32_t* __restrict__ ids, float* __restrict__ logp, float* __restrict__ lse) {
    const float L = lse_lanes(mx, sm);
    for (int j = 0; j < k; ++j) {
        float wv = tv[0];
        int wi = ti[0];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(wv, off, 64);
            const int oi = __shfl_xor(wi, off, 64);
            if (better(ov, oi, wv, wi)) {
                wv = ov;
                wi = oi;
            }
        }
        if (ti[0] == wi) {
#pragma unroll
            for (int q = 0; q + 1 < K; ++q) {
                tv[q] = tv[q + 1];
                ti[q] = ti[q + 1];
            }
            tv[K - 1] = -INFINITY;
            ti[K - 1] = NOIDX;
        }
        if (lane == 0) {
            ids[row * k + j] = wi;
            logp[row * k + j] = wv - L;
        }
    }
    if (lane == 0 && lse) lse[row] = L;
}

// the fused form's policy: a sorted list of K pairs per lane; partials [M, HP, 2] x (K values | K indices | (max, sum))
struct TopkParts {
    float* part_val;
    int32_t* part_idx;
    float* part_ms;
};
template <int K>
struct TopkScan {
    typedef TopkParts Args;
    // vectors, not arrays: members of a struct, arrays are taken apart into scalars only after unrolling, which the compiler then
    // pairs up again with copies in every insert; vectors stay whole as the arrays of a kernel's own locals do (k = 8: +0.8 % otherwise)
    float tv __attribute__((ext_vector_type(K)));
    int ti __attribute__((ext_vector_type(K)));
    __device__ __forceinline__ TopkScan() { topk_clear<K>(tv, ti); }
    __device__ __forceinline__ void begin(const Args&, int64_t, int64_t, int) { topk_clear<K>(tv, ti); }
    __device__ __forceinline__ void block(const float (&x)[16], int col0, int nv) {
#pragma unroll
        for (int c = 0; c < 16; ++c)
            if (c < nv && better(x[c], col0 + c, tv[K - 1], ti[K - 1])) topk_insert<K>(tv, ti, x[c], col0 + c);
    }
    __device__ __forceinline__ void leave(const Args& a, int64_t base, const LseState& lse) const {
#pragma unroll
        for (int q = 0; q < K; ++q) {
            a.part_val[base * K + q] = tv[q];
            a.part_idx[base * K + q] = ti[q];
        }
        a.part_ms[base * 2] = lse.mx;
        a.part_ms[base * 2 + 1] = lse.sm;
    }
};

// one wave per row: lane p < 2 x (workgroups on the row's block) takes list p
template <int K>
__global__ __launch_bounds__(256) void head_topk_merge_kernel(const float* __restrict__ part_val, const int32_t* __restrict__ part_idx,
                                                             const float* __restrict__ part_ms, int64_t M, int NT, int64_t U, int64_t G,
                                                             int HP, int k, int32_t* __restrict__ ids, float* __restrict__ logp,
                                                             float* __restrict__ lse) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int64_t m = row / HS_BM;
    const int P = 2 * (int)(block_of(m * NT + NT - 1, U, G) - block_of(m * NT, U, G) + 1);
    float tv[K], mx = -INFINITY, sm = 0.f;
    int ti[K];
    topk_clear<K>(tv, ti);
    if (lane < P) {
        const int64_t base = row * HP * 2 + lane;
#pragma unroll
        for (int q = 0; q < K; ++q) {
            tv[q] = part_val[base * K + q];
            ti[q] = part_idx[base * K + q];
        }
        mx = part_ms[base * 2];
        sm = part_ms[base * 2 + 1];
    }
    wave_finish<K>(tv, ti, mx, sm, k, row, lane, ids, logp, lse);
}

// top-k and log-sum-exp of the rows of a materialised matrix, one wave per row: lane l walks columns l, l + 64, ...
template <int K>
__global__ __launch_bounds__(256) void topk_lse_rows_kernel(const float* __restrict__ x, int64_t M, int N, int k,
                                                           int32_t* __restrict__ ids, float* __restrict__ logp, float* __restrict__ lse) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* xr = x + row * N;
    float tv[K], mx = -INFINITY, sm = 0.f;
    int ti[K];
    topk_clear<K>(tv, ti);
    for (int i = lane; i < N; i += 64) {
        const float v = xr[i];
        if (v > mx) {
            sm = sm * __expf(mx - v) + 1.f;       // (mx == -inf: sm is 0)
            mx = v;
        } else if (mx > -INFINITY) {
            sm += __expf(v - mx);
        }
        if (better(v, i, tv[K - 1], ti[K - 1])) topk_insert<K>(tv, ti, v, i);
    }
    wave_finish<K>(tv, ti, mx, sm, k, row, lane, ids, logp, lse);
}

#define TOPK_DISPATCH(K_, CALL)                       \
    switch (K_) {                                     \
        case 1: { constexpr int KK = 1; CALL; } break;   \
        case 2: { constexpr int KK = 2; CALL; } break;   \
        case 4: { constexpr int KK = 4; CALL; } break;   \
        case 8: { constexpr int KK = 8; CALL; } break;   \
        default: { constexpr int KK = 16; CALL; } break; \
    }

int launch_topk_lse_rows(const float* x, int64_t M, int N, int k, int32_t* ids, float* logp, float* lse, hipStream_t s) {
    ProfScope prof(PROF_OTHER, (double)M * N * 4.0, s);
    TOPK_DISPATCH(list_len(k), hipLaunchKernelGGL(topk_lse_rows_kernel<KK>, dim3((unsigned)cdiv(M, 4)), dim3(256), 0, s, x, M, N, k, ids,
                                                  logp, lse));
    TAL_CHECK_LAUNCH("topk_lse_rows");
    return TAL_OK;
}

// the fused launch the plan describes
int launch_head_topk(const HeadLaunch& p, const float* feat, const float* w, const float* b, int64_t M, int S, int k, int32_t* ids,
                     float* logp, float* lse, void* workspace, hipStream_t s) {
    char* ws = reinterpret_cast<char*>(workspace);
    const TopkParts parts = {reinterpret_cast<float*>(ws + p.off[0]), reinterpret_cast<int32_t*>(ws + p.off[1]), reinterpret_cast<float*>(ws + p.off[2])};
    const int64_t grid = p.run.grid;
    {
        ProfScope prof(PROF_GEMM, 2.0 * (double)M * (double)S * TK, s);
        TOPK_DISPATCH(p.K, hipLaunchKernelGGL((head_stream_kernel<TK, TopkScan<KK>>), dim3((unsigned)grid), dim3(256), 0, s, feat, (int64_t)TK, w, b,
                                              M, S, p.NT, p.U, parts, p.run.hp));
        TAL_CHECK_LAUNCH("head_topk");
    }
    ProfScope prof(PROF_OTHER, (double)p.need, s);
    TOPK_DISPATCH(p.K, hipLaunchKernelGGL(head_topk_merge_kernel<KK>, dim3((unsigned)cdiv(M, 4)), dim3(256), 0, s, parts.part_val, parts.part_idx, parts.part_ms, M, p.NT, p.U, grid,
                                          p.run.hp, k, ids, logp, lse));
    TAL_CHECK_LAUNCH("head_topk(merge)");
    return TAL_OK;
}

}  // namespace

}  // namespace tal

using namespace tal;

extern "C" size_t tal_spk_topk_workspace_bytes(int64_t M, int S, int E, int k) { return head_query_bytes(head_call(HE_TOPK, M, S, E, E, k, E)); }

extern "C" int tal_spk_topk_fwd(const float* feat, int64_t M, int E, const float* w_logit, const float* b_logit, int S, int k,
                                int32_t* ids, float* logp, float* lse, void* workspace, size_t workspace_bytes, void* stream) {
    TAL_CHECK_ARG(M >= 0 && E > 0 && S > 0, "tal_spk_topk_fwd: bad shape (M=%lld, E=%d, S=%d)", (long long)M, E, S);
    TAL_CHECK_ARG(k >= 1 && k <= TAL_TOPK_MAX && k <= S, "tal_spk_topk_fwd: k=%d outside 1..min(%d, S=%d)", k, TAL_TOPK_MAX, S);
    if (M == 0) return TAL_OK;
    TAL_CHECK_ARG(feat && w_logit && ids && logp, "tal_spk_topk_fwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const HeadCall c = head_call(HE_TOPK, M, S, E, E, k, E, 0, feat, w_logit, w_logit, workspace, workspace_bytes);
    const HeadLaunch p = head_call_plan(c);
    if (p.refusal) return head_refused(c, p);
    if (p.fused) return launch_head_topk(p, feat, w_logit, b_logit, M, S, k, ids, logp, lse, workspace, s);
    // the logits of a chunk of rows through the dense layer, then the row kernel
    float* logits = reinterpret_cast<float*>(workspace);
    return for_row_chunks(M, p.chunk, [&](int64_t r0, int64_t rows) {
        const int rc = launch_linear(feat + r0 * E, w_logit, b_logit, nullptr, 0.f, 0, rows, S, E, logits, s);
        return rc ? rc : launch_topk_lse_rows(logits, rows, S, k, ids + r0 * k, logp + r0 * k, lse ? lse + r0 : nullptr, s);
    });
}

extern "C" int tal_topk_lse_rows(const float* x, int64_t M, int N, int k, int32_t* ids, float* logp, float* lse, void* stream) {
    TAL_CHECK_ARG(M >= 0 && N > 0, "tal_topk_lse_rows: bad shape (M=%lld, N=%d)", (long long)M, N);
    TAL_CHECK_ARG(k >= 1 && k <= TAL_TOPK_MAX && k <= N, "tal_topk_lse_rows: k=%d outside 1..min(%d, N=%d)", k, TAL_TOPK_MAX, N);
    if (M == 0) return TAL_OK;
    TAL_CHECK_ARG(x && ids && logp, "tal_topk_lse_rows: null pointer");
    return launch_topk_lse_rows(x, M, N, k, ids, logp, lse, (hipStream_t)stream);
}
