// Teacher-forced scoring without the logits: per row r of a head z[r, s] = feat[r, :] . W[s, :] + b[s]
//   lse[r] = log sum_s exp(z[r, s]),  nll[r] = lse[r] - z[r, target[r]],  top1[r] = arg-max_s z[r, s] (first index among equal values)
// The sibling of csrc/head_topk.hip: the same stream of logits through registers and the same online log-sum-exp, with a target
// gather and a running arg-max in place of the running top-k.  A target is only ever COMPARED with the column index a logit
// belongs to, never used as an address: target < 0 skips the row's loss (nll = 0), target >= N finds no column (nll = +inf).
//
// FUSED FORM (E = 64: the factorised LM head; E = 128: the speaker head).  The skeleton is head_topk_kernel, templated on E: each
// wave keeps its 32 x E feature strip as E / 8 MFMA-ready fragments, W streams through LDS in 128-column N tiles (double-buffered
// 128 x 32 chunks in the dense layers' XOR-swizzled image, one barrier per chunk, staged with ordinary global loads into registers
// under the MFMAs of the chunk before and LDS writes -- no LDS-DMA, nothing in flight at a barrier that the compiler does not wait for
// by itself), the products are v_mfma_f32_32x32x2_f32 (exact fp32), work is cut into equal runs of (row block, N tile) units.
// After an N tile's MFMAs the wave writes its logits (+ bias) to a wave-private LDS tile one 32 x 32 sub-tile at a time (row pitch 33)
// and TWO LANES PER ROW scan 16 columns each: block maximum first, ONE rescale of the running (max, sum exp(z - max)) per block, then
// the exps, the running arg-max, and the target's logit when the target's column is among the 16 -- the same value the sum saw, so
// nll >= 0 up to rounding and lse - nll is the logit.
// A workgroup leaves, per row, per slot (its rank among the workgroups of that row block) and per lane half, (max, sum, best value,
// best index, target logit or -inf = "not seen"); xent_merge_kernel -- one wave per row, one partial per lane -- adds the sums
// rescaled to the common maximum in a fixed butterfly order, takes the best (value, index) and the one target logit that was seen:
// bit-identical call after call.
//
// GENERIC FORM (any E the dense layer takes): the logits of a chunk of rows go to the workspace through the dense layer (<= 64 MiB),
// xent_lse_rows_kernel -- one wave per row -- reads them back.  The same kernel is tal_xent_lse_rows.
#include <math.h>

#include "common.h"

namespace tal {

namespace {

constexpr int XBM = 128, XBN = 128, XNSUB = 4;
constexpr int XP_MAX = 16;          // most workgroup slots per row
constexpr int XPITCH = 33;          // row pitch (floats) of a wave's 32 x 32 logit tile
constexpr int NOIDX = 0x7fffffff;
constexpr size_t GENERIC_WS_MAX = (size_t)64 << 20;

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

// workgroup whose run [b U / G, (b + 1) U / G) contains unit u
__host__ __device__ inline int64_t block_of(int64_t u, int64_t U, int64_t G) {
    int64_t b = u * G / U;
    while ((b + 1) * U / G <= u) ++b;
    while (b * U / G > u) --b;
    return b;
}

// arg-max order: value descending, index ascending among equal values (the empty entry (-inf, NOIDX) ranks below every column)
__device__ __forceinline__ bool better(float v, int i, float tv, int ti) { return v > tv || (v == tv && i < ti); }

// the column a target can match: -1 (no column) for a skipped row and for a target past the head
__device__ __forceinline__ int target_col(int64_t t, int N) { return t >= 0 && t < (int64_t)N ? (int)t : -1; }

// One row per wave, one partial per lane (empty: (-inf, 0), (-inf, NOIDX), -inf): lse from the sums rescaled to the common
// maximum, the best (value, index), the target's logit (at most one lane saw it: the maximum over the lanes is that value).
__device__ __forceinline__ void wave_finish(float mx, float sm, float bv, int bi, float tz, int64_t tgt, int64_t row, int lane,
                                            float* __restrict__ nll, float* __restrict__ lse, int32_t* __restrict__ top1) {
    float g = mx;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) g = fmaxf(g, __shfl_xor(g, off, 64));
    float t = mx > -INFINITY ? sm * expf(mx - g) : 0.f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);     // (a fixed tree: every lane holds the same sum)
    const float L = g + logf(t);
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

template <int E>
__global__ __launch_bounds__(256, 2) void xent_kernel(const float* __restrict__ feat, int64_t ldf, const float* __restrict__ W,
                                                     const float* __restrict__ bias, const int64_t* __restrict__ target, int64_t M,
                                                     int S, int NT, int64_t U, float* __restrict__ part_f,
                                                     int32_t* __restrict__ part_i, int HP) {
    __shared__ __attribute__((aligned(16))) float wbuf[2 * XBN * 32];      // 32,768 B
    __shared__ float tile[4 * 32 * XPITCH];                                // 16,896 B
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
            const int col = n * XBN + srow + 32 * i;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            pre[i] = col < S ? *reinterpret_cast<const f32x4*>(W + (int64_t)col * E + kt * 32 + scol * 4) : zero;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(wbuf + buf * (XBN * 32) + sdst + i * (32 * 32)) = pre[i];
    };

    f32x4 a[E / 8];           // this wave's 32 x E strip: a[kk] = A[row, 8 kk + 4 (lane >> 5) .. + 3]
    f32x16 acc[XNSUB];
#pragma unroll
    for (int j = 0; j < XNSUB; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    // scan state of this lane: row (lane & 31) of the wave's strip, columns [16 (lane >> 5), + 16) of every 32-column sub-tile
    float mx = -INFINITY, sm = 0.f, bv = -INFINITY, tz = -INFINITY;
    int bi = NOIDX, tcol = -1;
    float* mytile = tile + w * (32 * XPITCH);

    // (E / 32 is even: the chunk after a unit's last lands in buffer 0, where the next unit's kt = 0 looks for it)
    static_assert((E / 32) % 2 == 0, "the double buffer's parity needs an even number of chunks per unit");
    fetch((int)(u0 % NT), 0);
    stash(0);
    for (int64_t u = u0; u < u1; ++u) {
        const int64_t m = u / NT;
        const int n = (int)(u - m * NT);
        const int64_t row0 = m * XBM + w * 32;
        if (u == u0 || n == 0) {
            int64_t r = row0 + frow;
            tcol = r < M ? target_col(target[r], S) : -1;
            r = r < M ? r : M - 1;
            const float* ap = feat + r * ldf + 4 * fhalf;
#pragma unroll
            for (int kk = 0; kk < E / 8; ++kk) a[kk] = *reinterpret_cast<const f32x4*>(ap + 8 * kk);
            mx = -INFINITY;
            sm = 0.f;
            bv = -INFINITY;
            bi = NOIDX;
            tz = -INFINITY;
        }
        float bcol[XNSUB];
#pragma unroll
        for (int j = 0; j < XNSUB; ++j) {
            const int col = n * XBN + j * 32 + frow;
            bcol[j] = bias && col < S ? bias[col] : 0.f;
        }
#pragma unroll
        for (int kt = 0; kt < E / 32; ++kt) {
            const int buf = kt & 1;
            __syncthreads();      // chunk (n, kt) is in LDS (written before this barrier); everyone is done with the other buffer
            const bool more = kt + 1 < E / 32 || u + 1 < u1;
            if (more) {
                if (kt + 1 < E / 32)
                    fetch(n, kt + 1);
                else
                    fetch((int)((u + 1) % NT), 0);
            }
            const float* Bs = wbuf + buf * (XBN * 32) + frow * 32;
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) {
                const int sl = ((2 * k4 + fhalf) ^ fsw) * 4;
                f32x4 fb[XNSUB];
#pragma unroll
                for (int j = 0; j < XNSUB; ++j) fb[j] = *reinterpret_cast<const f32x4*>(Bs + j * 32 * 32 + sl);
                const f32x4 fa = a[kt * 4 + k4];
#pragma unroll
                for (int j = 0; j < XNSUB; ++j) {
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
        for (int j = 0; j < XNSUB; ++j) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                mytile[((e & 3) + 8 * (e >> 2) + 4 * fhalf) * XPITCH + frow] = acc[j][e] + bcol[j];
                acc[j][e] = 0.f;
            }
            // the tile is this wave's own: its LDS instructions execute in order, the fences keep the compiler from reordering them
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int col0 = n * XBN + j * 32 + fhalf * 16;
            float x[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) x[c] = mytile[frow * XPITCH + fhalf * 16 + c];
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
            for (int c = 0; c < 16; ++c) {
                if (c < nv && better(x[c], col0 + c, bv, bi)) {
                    bv = x[c];
                    bi = col0 + c;
                }
                if (col0 + c == tcol) tz = x[c];        // (tcol < S: an existing column)
            }
        }
        if (n == NT - 1 || u == u1 - 1) {
            // this workgroup's share of row block m is complete
            const int slot = (int)((int64_t)blockIdx.x - block_of(m * NT, U, G));
            const int64_t row = row0 + frow;
            if (row < M) {
                const int64_t base = (row * HP + slot) * 2 + fhalf;
                f32x4 p = {mx, sm, bv, tz};
                *reinterpret_cast<f32x4*>(part_f + base * 4) = p;
                part_i[base] = bi;
            }
        }
    }
}

// one wave per row: lane p < 2 x (workgroups on the row's block) takes partial p
__global__ __launch_bounds__(256) void xent_merge_kernel(const float* __restrict__ part_f, const int32_t* __restrict__ part_i,
                                                        const int64_t* __restrict__ target, int64_t M, int NT, int64_t U, int64_t G,
                                                        int HP, float* __restrict__ nll, float* __restrict__ lse,
                                                        int32_t* __restrict__ top1) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int64_t m = row / XBM;
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

// workgroups of the fused launch and slots per row.  A run is U / grid units or one more; a row block's NT units then meet at most
// 1 + ceil((NT - 1) / (U / grid)) runs.  Default: two workgroups per CU; runs never shorter than NT / 15 tiles (XP_MAX slots).
void xent_plan(int64_t M, int S, int64_t& grid, int& hp) {
    const int64_t nt = cdiv(S, XBN), units = cdiv(M, XBM) * nt, lmin = cdiv(nt, (int64_t)(XP_MAX - 1));
    int64_t g = opt(OPT_XENT_GRID) > 0 ? opt(OPT_XENT_GRID) : 2 * (int64_t)device_cus();
    if (g > units) g = units;
    if (units / g < lmin) g = units / lmin;
    const int64_t len = units / g, slots = 1 + cdiv(nt - 1, len);
    grid = g;
    hp = (int)(slots < g ? slots : g);
}

// per row, slot and lane half: (max, sum, best value, target logit) and the best index
size_t fused_ws_bytes(int64_t M, int S) {
    int64_t grid;
    int hp;
    xent_plan(M, S, grid, hp);
    return (size_t)M * hp * 2 * 20;
}

int64_t generic_chunk_rows(int64_t M, int S) {
    int64_t rows = (int64_t)(GENERIC_WS_MAX / ((size_t)S * 4));
    rows = rows < 1 ? 1 : rows;
    return rows < M ? rows : M;
}

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
    const int NT = (int)cdiv(S, XBN);
    const int64_t U = cdiv(M, XBM) * NT;
    int64_t grid;
    int hp;
    xent_plan(M, S, grid, hp);
    float* pf = reinterpret_cast<float*>(workspace);
    int32_t* pi = reinterpret_cast<int32_t*>(pf + (size_t)M * hp * 2 * 4);
    {
        ProfScope prof(PROF_GEMM, 2.0 * (double)M * (double)S * E, s);
        if (E == 64)
            hipLaunchKernelGGL(xent_kernel<64>, dim3((unsigned)grid), dim3(256), 0, s, feat, ldf, w, b, target, M, S, NT, U, pf, pi, hp);
        else
            hipLaunchKernelGGL(xent_kernel<128>, dim3((unsigned)grid), dim3(256), 0, s, feat, ldf, w, b, target, M, S, NT, U, pf, pi, hp);
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
        int rc;
        if (ldf == E) {
            rc = launch_linear(feat + r0 * ldf, w, bias, nullptr, 0.f, 0, rows, N, E, logits, s);
        } else {
            GemmArgs g = {};
            g.A = feat + r0 * ldf; g.W = w; g.bias = bias; g.Y = logits; g.M = rows; g.N = N; g.K = E;
            g.lda = ldf; g.ldw = E; g.ldy = N; g.ldres = N; g.nb2 = 1;
            rc = launch_gemm(g, 0, 1, s);
        }
        if (rc) return rc;
        rc = launch_xent_lse_rows(logits, rows, N, target + r0, nll + r0, lse ? lse + r0 : nullptr, top1 ? top1 + r0 : nullptr, s);
        if (rc) return rc;
    }
    return TAL_OK;
}

size_t lm_proj_bytes(int64_t M, int E0) { return ((size_t)M * E0 * sizeof(float) + 15) & ~(size_t)15; }

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
    const size_t head = lm_proj_bytes(M, E0);
    if (!workspace || workspace_bytes < head) {
        set_error("tal_lm_xent_fwd: workspace %zu < %zu bytes", workspace ? workspace_bytes : (size_t)0, head);
        return TAL_ENOMEM;
    }
    float* t = reinterpret_cast<float*>(workspace);
    GemmArgs g = {};
    g.nb2 = 1;
    g.A = h; g.W = proj_t; g.Y = t; g.M = M; g.N = E0; g.K = D; g.lda = ldh; g.ldw = D; g.ldy = E0;
    // (the checks of the second stage run before the projection is launched: a refused call launches nothing)
    const int form = opt(OPT_XENT_FORM);
    TAL_CHECK_ARG(form != 2 || fused_possible(t, E0, emb, E0),
                  "tal_lm_xent_fwd: the fused form needs E0 == 64 or 128 and 16-byte aligned operands (E0=%d)", E0);
    const bool fused = fused_by_shape(M, E0) && fused_possible(t, E0, emb, E0);
    const size_t need = head + (fused ? fused_ws_bytes(M, V) : (size_t)V * 4);
    if (workspace_bytes < need) {
        set_error("tal_lm_xent_fwd: workspace %zu < %zu bytes", workspace_bytes, need);
        return TAL_ENOMEM;
    }
    int rc = launch_gemm(g, 0, 1, s);
    if (rc) return rc;
    return xent_rows("tal_lm_xent_fwd", t, M, E0, E0, emb, nullptr, V, target, nll, lse, top1, reinterpret_cast<char*>(workspace) + head,
                     workspace_bytes - head, s);
}
