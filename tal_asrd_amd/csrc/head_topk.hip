// Per-frame top-k speaker posteriors of the diarization head without the logits:
//   z[r, s] = feat[r, :] . W[s, :] + b[s],  lse[r] = log sum_s exp(z[r, s]),
//   ids[r, 0..k) = the k largest z[r, :] (value descending, index ascending among equal values),  logp[r, j] = z[r, ids[r, j]] - lse[r]
// The sibling of csrc/head.hip's arg-max: the same stream of logits through registers, a running top-k and an online
// log-sum-exp instead of a running maximum.
//
// FUSED FORM (E = 128).  The skeleton is head_argmax_kernel<false>: each wave keeps its 32 x 128 feature strip as 16 MFMA-ready
// fragments, W streams through LDS in 128-column N tiles (double-buffered 128 x 32 chunks in the dense layers' XOR-swizzled image,
// one barrier per chunk), the products are v_mfma_f32_32x32x2_f32 (exact fp32), work is cut into equal runs of (row block, N tile)
// units.  Two things differ:
//   * W is staged with ordinary global loads into registers (issued under the MFMAs of the chunk before) and LDS writes -- no
//     LDS-DMA, so there is no load in flight at a barrier that the compiler does not wait for by itself.
//   * A running top-k per accumulator element would take 16 rows x k x (value, index) registers per lane.  Instead, after an N
//     tile's MFMAs the wave writes its logits (+ bias) to a wave-private LDS tile one 32 x 32 sub-tile at a time (row pitch 33:
//     the 32 lanes of a half wave, which read one column of 32 different rows, hit 32 different banks) and TWO LANES PER ROW scan 16
//     columns each: block maximum first, ONE rescale of the running (max, sum exp(z - max)) per block, then the exps, then the
//     sorted top-k, compared against its k-th entry first (an insert is rare after the first tiles).  Register cost: 2 k + 2,
//     independent of the tile.
// A workgroup leaves, per row, per slot (its rank among the workgroups of that row block) and per lane half, k (value, index)
// pairs and (max, sum); head_topk_merge_kernel -- one wave per row, one list per lane -- pops the k winners in order and adds the
// sums, rescaled to the common maximum, in a fixed butterfly order: bit-identical call after call.
//
// GENERIC FORM (any E the dense layer takes): the logits of a chunk of rows go to the workspace through launch_linear (<= 64 MiB),
// topk_lse_rows_kernel -- one wave per row -- reads them back.  The same kernel is tal_topk_lse_rows.
#include <math.h>

#include "common.h"

namespace tal {

namespace {

constexpr int TK = 128;             // feature width (K)
constexpr int TBM = 128, TBN = 128, TNSUB = 4;
constexpr int TP_MAX = 16;          // most workgroup slots per row
constexpr int TPITCH = 33;          // row pitch (floats) of a wave's 32 x 32 logit tile
constexpr int NOIDX = 0x7fffffff;
constexpr size_t GENERIC_WS_MAX = (size_t)64 << 20;

// rows at and above which auto dispatch takes the fused form for E = 128: the smallest row count of the sweep in
// profiles/head_topk.txt at which it measured faster than the generic form (2048 rows: generic 0.114 ms, fused 0.126;
// 3751 rows: 0.225 / 0.176)
constexpr int64_t FUSED_FROM_ROWS = 3751;

// workgroup whose run [b U / G, (b + 1) U / G) contains unit u
__host__ __device__ inline int64_t block_of(int64_t u, int64_t U, int64_t G) {
    int64_t b = u * G / U;
    while ((b + 1) * U / G <= u) ++b;
    while (b * U / G > u) --b;
    return b;
}

// the order of the results: value descending, index ascending among equal values (-inf columns included; the empty entry
// (-inf, NOIDX) ranks below every column)
__device__ __forceinline__ bool better(float v, int i, float tv, int ti) { return v > tv || (v == tv && i < ti); }

template <int K>
__device__ __forceinline__ void topk_clear(float (&tv)[K], int (&ti)[K]) {
#pragma unroll
    for (int q = 0; q < K; ++q) {
        tv[q] = -INFINITY;
        ti[q] = NOIDX;
    }
}

// insert into the sorted list: the newcomer takes the first place it is better than, everything behind moves down one
template <int K>
__device__ __forceinline__ void topk_insert(float (&tv)[K], int (&ti)[K], float v, int i) {
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
    float g = mx;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) g = fmaxf(g, __shfl_xor(g, off, 64));
    float t = mx > -INFINITY ? sm * expf(mx - g) : 0.f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);     // (a fixed tree: every lane holds the same sum)
    const float L = g + logf(t);
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

template <int K>
__global__ __launch_bounds__(256, 2) void head_topk_kernel(const float* __restrict__ feat, const float* __restrict__ W,
                                                          const float* __restrict__ bias, int64_t M, int S, int NT, int64_t U,
                                                          float* __restrict__ part_val, int32_t* __restrict__ part_idx,
                                                          float* __restrict__ part_ms, int HP) {
    __shared__ __attribute__((aligned(16))) float wbuf[2 * TBN * 32];      // 32,768 B
    __shared__ float tile[4 * 32 * TPITCH];                                // 16,896 B
    const int64_t G = gridDim.x;
    const int64_t u0 = (int64_t)blockIdx.x * U / G, u1 = ((int64_t)blockIdx.x + 1) * U / G;
    if (u0 >= u1) return;
    const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
    const int frow = lane & 31, fsw = (frow >> 1) & 7, fhalf = lane >> 5;     // swizzle: see gemm_glds_kernel

    // chunk (n, kt): W rows [128 n, 128 n + 128), k in [32 kt, 32 kt + 32): thread t moves the 16-byte column t & 7 of rows
    // (t >> 3) + 32 i, i < 4 (8 threads = one 128-byte row segment); rows past S are zeros (their columns are skipped below)
    const int srow = tid >> 3, scol = tid & 7;
    const int sdst = srow * 32 + ((scol ^ ((srow >> 1) & 7)) * 4);            // ((srow + 32 i) >> 1) & 7 == (srow >> 1) & 7
    f32x4 pre[4];
    auto fetch = [&](int n, int kt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int col = n * TBN + srow + 32 * i;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            pre[i] = col < S ? *reinterpret_cast<const f32x4*>(W + (int64_t)col * TK + kt * 32 + scol * 4) : zero;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(wbuf + buf * (TBN * 32) + sdst + i * (32 * 32)) = pre[i];
    };

    f32x4 a[TK / 8];          // this wave's 32 x 128 strip: a[kk] = A[row, 8 kk + 4 (lane >> 5) .. + 3]
    f32x16 acc[TNSUB];
#pragma unroll
    for (int j = 0; j < TNSUB; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    // scan state of this lane: row (lane & 31) of the wave's strip, columns [16 (lane >> 5), + 16) of every 32-column sub-tile
    float tv[K], mx = -INFINITY, sm = 0.f;
    int ti[K];
    topk_clear<K>(tv, ti);
    float* mytile = tile + w * (32 * TPITCH);

    fetch((int)(u0 % NT), 0);
    stash(0);
    for (int64_t u = u0; u < u1; ++u) {
        const int64_t m = u / NT;
        const int n = (int)(u - m * NT);
        const int64_t row0 = m * TBM + w * 32;
        if (u == u0 || n == 0) {
            int64_t r = row0 + frow;
            r = r < M ? r : M - 1;
            const float* ap = feat + r * TK + 4 * fhalf;
#pragma unroll
            for (int kk = 0; kk < TK / 8; ++kk) a[kk] = *reinterpret_cast<const f32x4*>(ap + 8 * kk);
            topk_clear<K>(tv, ti);
            mx = -INFINITY;
            sm = 0.f;
        }
        float bv[TNSUB];
#pragma unroll
        for (int j = 0; j < TNSUB; ++j) {
            const int col = n * TBN + j * 32 + frow;
            bv[j] = bias && col < S ? bias[col] : 0.f;
        }
#pragma unroll
        for (int kt = 0; kt < TK / 32; ++kt) {
            const int buf = kt & 1;
            __syncthreads();      // chunk (n, kt) is in LDS (written before this barrier); everyone is done with the other buffer
            const bool more = kt + 1 < TK / 32 || u + 1 < u1;
            if (more) {
                if (kt + 1 < TK / 32)
                    fetch(n, kt + 1);
                else
                    fetch((int)((u + 1) % NT), 0);
            }
            const float* Bs = wbuf + buf * (TBN * 32) + frow * 32;
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) {
                const int sl = ((2 * k4 + fhalf) ^ fsw) * 4;
                f32x4 fb[TNSUB];
#pragma unroll
                for (int j = 0; j < TNSUB; ++j) fb[j] = *reinterpret_cast<const f32x4*>(Bs + j * 32 * 32 + sl);
                const f32x4 fa = a[kt * 4 + k4];
#pragma unroll
                for (int j = 0; j < TNSUB; ++j) {
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.x, fb[j].x, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.y, fb[j].y, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.z, fb[j].z, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.w, fb[j].w, acc[j], 0, 0, 0);
                }
            }
            if (more) stash(buf ^ 1);     // (read last in front of this iteration's barrier)
        }
        // scan: accumulator element e of lane l is row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column 32 j + (l & 31) of the strip
#pragma unroll
        for (int j = 0; j < TNSUB; ++j) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                mytile[((e & 3) + 8 * (e >> 2) + 4 * fhalf) * TPITCH + frow] = acc[j][e] + bv[j];
                acc[j][e] = 0.f;
            }
            // the tile is this wave's own: its LDS instructions execute in order, the fences keep the compiler from reordering them
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int col0 = n * TBN + j * 32 + fhalf * 16;
            float x[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) x[c] = mytile[frow * TPITCH + fhalf * 16 + c];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int nv = S - col0;          // columns [col0, col0 + nv) exist
            float cm = -INFINITY;
#pragma unroll
            for (int c = 0; c < 16; ++c)
                if (c < nv) cm = fmaxf(cm, x[c]);
            if (cm > mx) {                    // (mx == -inf: sm is 0 and stays 0)
                sm *= __expf(mx - cm);
                mx = cm;
            }
            if (mx > -INFINITY) {             // (a -inf column adds exp(-inf) = 0; all -inf so far: nothing to add)
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (c < nv) sm += __expf(x[c] - mx);
            }
#pragma unroll
            for (int c = 0; c < 16; ++c)
                if (c < nv && better(x[c], col0 + c, tv[K - 1], ti[K - 1])) topk_insert<K>(tv, ti, x[c], col0 + c);
        }
        if (n == NT - 1 || u == u1 - 1) {
            // this workgroup's share of row block m is complete
            const int slot = (int)((int64_t)blockIdx.x - block_of(m * NT, U, G));
            const int64_t row = row0 + frow;
            if (row < M) {
                const int64_t base = (row * HP + slot) * 2 + fhalf;
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    part_val[base * K + q] = tv[q];
                    part_idx[base * K + q] = ti[q];
                }
                part_ms[base * 2] = mx;
                part_ms[base * 2 + 1] = sm;
            }
        }
    }
}

// one wave per row: lane p < 2 x (workgroups on the row's block) takes list p
template <int K>
__global__ __launch_bounds__(256) void head_topk_merge_kernel(const float* __restrict__ part_val, const int32_t* __restrict__ part_idx,
                                                             const float* __restrict__ part_ms, int64_t M, int NT, int64_t U, int64_t G,
                                                             int HP, int k, int32_t* __restrict__ ids, float* __restrict__ logp,
                                                             float* __restrict__ lse) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int64_t m = row / TBM;
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

int list_len(int k) {       // the kernels keep lists of 1, 2, 4, 8 or 16 entries
    int K = 1;
    while (K < k) K *= 2;
    return K;
}

// workgroups of the fused launch and slots per row.  A run is U / grid units or one more; a row block's NT units then meet at most
// 1 + ceil((NT - 1) / (U / grid)) runs.  Default: two workgroups per CU; runs never shorter than NT / 15 tiles (TP_MAX slots).
void head_topk_plan(int64_t M, int S, int64_t& grid, int& hp) {
    const int64_t nt = cdiv(S, TBN), units = cdiv(M, TBM) * nt, lmin = cdiv(nt, (int64_t)(TP_MAX - 1));
    int64_t g = opt(OPT_HEAD_TOPK_GRID) > 0 ? opt(OPT_HEAD_TOPK_GRID) : 2 * (int64_t)device_cus();
    if (g > units) g = units;
    if (units / g < lmin) g = units / lmin;
    const int64_t len = units / g, slots = 1 + cdiv(nt - 1, len);
    grid = g;
    hp = (int)(slots < g ? slots : g);
}

size_t fused_ws_bytes(int64_t M, int S, int k) {
    int64_t grid;
    int hp;
    head_topk_plan(M, S, grid, hp);
    return (size_t)M * hp * 2 * ((size_t)list_len(k) * 8 + 8);
}

int64_t generic_chunk_rows(int64_t M, int S) {
    int64_t rows = (int64_t)(GENERIC_WS_MAX / ((size_t)S * 4));
    rows = rows < 1 ? 1 : rows;
    return rows < M ? rows : M;
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

int launch_head_topk(const float* feat, const float* w, const float* b, int64_t M, int S, int k, int32_t* ids, float* logp, float* lse,
                     void* workspace, hipStream_t s) {
    const int NT = (int)cdiv(S, TBN), K = list_len(k);
    const int64_t U = cdiv(M, TBM) * NT;
    int64_t grid;
    int hp;
    head_topk_plan(M, S, grid, hp);
    float* pv = reinterpret_cast<float*>(workspace);
    int32_t* pi = reinterpret_cast<int32_t*>(pv + (size_t)M * hp * 2 * K);
    float* pms = reinterpret_cast<float*>(pi + (size_t)M * hp * 2 * K);
    {
        ProfScope prof(PROF_GEMM, 2.0 * (double)M * (double)S * TK, s);
        TOPK_DISPATCH(K, hipLaunchKernelGGL(head_topk_kernel<KK>, dim3((unsigned)grid), dim3(256), 0, s, feat, w, b, M, S, NT, U, pv, pi, pms, hp));
        TAL_CHECK_LAUNCH("head_topk");
    }
    ProfScope prof(PROF_OTHER, (double)M * hp * 2 * (K * 8.0 + 8.0), s);
    TOPK_DISPATCH(K, hipLaunchKernelGGL(head_topk_merge_kernel<KK>, dim3((unsigned)cdiv(M, 4)), dim3(256), 0, s, pv, pi, pms, M, NT, U, grid, hp, k,
                                        ids, logp, lse));
    TAL_CHECK_LAUNCH("head_topk(merge)");
    return TAL_OK;
}

bool fused_possible(const float* feat, const float* w, int E) {
    return E == TK && ((reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(w)) & 15) == 0;
}

}  // namespace

}  // namespace tal

using namespace tal;

extern "C" size_t tal_spk_topk_workspace_bytes(int64_t M, int S, int E, int k) {
    if (M <= 0 || S <= 0 || E <= 0 || k < 1 || k > TAL_TOPK_MAX) return 0;
    const size_t generic = (size_t)generic_chunk_rows(M, S) * (size_t)S * 4;
    const size_t fused = E == TK ? fused_ws_bytes(M, S, k) : 0;
    return generic > fused ? generic : fused;
}

extern "C" int tal_spk_topk_fwd(const float* feat, int64_t M, int E, const float* w_logit, const float* b_logit, int S, int k,
                                int32_t* ids, float* logp, float* lse, void* workspace, size_t workspace_bytes, void* stream) {
    TAL_CHECK_ARG(M >= 0 && E > 0 && S > 0, "tal_spk_topk_fwd: bad shape (M=%lld, E=%d, S=%d)", (long long)M, E, S);
    TAL_CHECK_ARG(k >= 1 && k <= TAL_TOPK_MAX && k <= S, "tal_spk_topk_fwd: k=%d outside 1..min(%d, S=%d)", k, TAL_TOPK_MAX, S);
    if (M == 0) return TAL_OK;
    TAL_CHECK_ARG(feat && w_logit && ids && logp, "tal_spk_topk_fwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int form = opt(OPT_HEAD_TOPK_FORM);
    TAL_CHECK_ARG(form != 2 || fused_possible(feat, w_logit, E),
                  "tal_spk_topk_fwd: the fused form needs E == %d and 16-byte aligned operands (E=%d)", TK, E);
    const bool fused = form == 2 || (form == 0 && fused_possible(feat, w_logit, E) && M >= FUSED_FROM_ROWS);
    const size_t need = fused ? fused_ws_bytes(M, S, k) : (size_t)generic_chunk_rows(M, S) * (size_t)S * 4;
    if (!workspace || workspace_bytes < need) {
        set_error("tal_spk_topk_fwd: workspace %zu < %zu bytes", workspace ? workspace_bytes : (size_t)0, need);
        return TAL_ENOMEM;
    }
    if (fused) return launch_head_topk(feat, w_logit, b_logit, M, S, k, ids, logp, lse, workspace, s);
    // the logits of a chunk of rows through the dense layer, then the row kernel
    const int64_t chunk = generic_chunk_rows(M, S);
    float* logits = reinterpret_cast<float*>(workspace);
    for (int64_t r0 = 0; r0 < M; r0 += chunk) {
        const int64_t rows = M - r0 < chunk ? M - r0 : chunk;
        int rc = launch_linear(feat + r0 * E, w_logit, b_logit, nullptr, 0.f, 0, rows, S, E, logits, s);
        if (rc) return rc;
        rc = launch_topk_lse_rows(logits, rows, S, k, ids + r0 * k, logp + r0 * k, lse ? lse + r0 : nullptr, s);
        if (rc) return rc;
    }
    return TAL_OK;
}

extern "C" int tal_topk_lse_rows(const float* x, int64_t M, int N, int k, int32_t* ids, float* logp, float* lse, void* stream) {
    TAL_CHECK_ARG(M >= 0 && N > 0, "tal_topk_lse_rows: bad shape (M=%lld, N=%d)", (long long)M, N);
    TAL_CHECK_ARG(k >= 1 && k <= TAL_TOPK_MAX && k <= N, "tal_topk_lse_rows: k=%d outside 1..min(%d, N=%d)", k, TAL_TOPK_MAX, N);
    if (M == 0) return TAL_OK;
    TAL_CHECK_ARG(x && ids && logp, "tal_topk_lse_rows: null pointer");
    return launch_topk_lse_rows(x, M, N, k, ids, logp, lse, (hipStream_t)stream);
}
