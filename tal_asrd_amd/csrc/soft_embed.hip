// Softmax-weighted embeddings without the logits: per row r of a head z[r, s] = feat[r, :] . W[s, :] + b[s]
//   lse[r] = log sum_s exp(z[r, s]),  out[r, :] = sum_s exp(z[r, s] - lse[r]) * values[s, :]      (values [N, D]; NULL: values = W)
// The streaming heads of csrc/head_stream.h reduce the posterior to a few scalars per row; here it is multiplied into a second
// matrix, so the kernel is a fused two-product (attention-shaped) one of its own: the queries are the rows of feat, the keys the
// rows of W, the values the rows of `values`.  It shares their run partition (csrc/head_plan.h) and host helpers.
//
// FUSED FORM ((E, D) = (64, 64) or (128, 128)).  A workgroup is four waves, a wave owns 32 queries; its 32 x E feature strip stays
// in registers as E / 8 MFMA-ready fragments (as in csrc/head_stream.h).  Keys stream through LDS in tiles of 64: the W tile, the values
// tile (unless values == W: then ONE image serves both products) and the tile's bias, double-buffered, one barrier per tile, staged
// with ordinary global loads into registers issued under the MFMAs of the tile before, then LDS writes -- no LDS-DMA, nothing in
// flight at a barrier that the compiler does not wait for by itself.  Every product is v_mfma_f32_32x32x2_f32 (exact fp32).
//   * The score tile is computed TRANSPOSED: A = the W tile (key on the MFMA row), B = the feature strip (query on the lane).  Lane l
//     then owns query l & 31, and accumulator element e of sub-tile j is key 32 j + (e & 3) + 8 (e >> 2) + 4 (l >> 5) of that query:
//     the row maximum and sum are in-lane reductions plus one exchange between the two lane halves, exp(z - m) happens in place.
//   * Those registers are directly the B operand of out^T[d, query] += values^T[d, key] * P[key, query]: k-step (j, e) of the second
//     product contracts the key pair (key(j, e, half 0), key(j, e, half 1)), and the values fragment is read with that same
//     permutation (the lane's half picks the key's LDS row).  P never crosses LDS.
//   * Output column order: lane row i of d-block db is column d = (D / 32) i + db, so a lane reads its D / 32 A operands of one key
//     as ONE 16- (8-) byte LDS read and stores D / 32 neighbouring columns of a partial at once.
//   * LDS image of a tile: row = key, pitch E floats, the 16-byte granule g of row k at slot g ^ (k & 15): the score product's reads
//     (16 consecutive keys, one granule) and the second product's (one key, 16 consecutive granules) both spread over all banks.
//   * Online softmax, the rescale at a change of the running maximum done for EVERYTHING at the old scale exactly once per tile and
//     before any P of the tile exists: all 64 scores of the tile first, then the new maximum, then f = exp(m_old - m_new) on the
//     output accumulators and the running sum, then P = exp(z - m_new), then the second product.  No deferred-rescale threshold.
//   Budget (E = D = 128): registers per lane 64 (feature strip) + 64 (output accumulators) + 32 (score tile) + 32 + 32 (W / values
//   tile in flight) + addresses ~ 240 of the 512 a wave has at one wave per SIMD; LDS 2 x (32 + 32) KiB + 512 B = 128.5 KiB of the
//   CU's 160 (64.5 KiB with values == W), i.e. one workgroup per CU.  A 128-key tile would double both the LDS image and the
//   registers in flight and fit neither.
// Work is cut into equal runs of (128-row block, 64-key tile) units (csrc/head_plan.h); a workgroup leaves, per row and per slot (its
// rank among the workgroups of that row block), (max, sum, out[D]) unnormalised; soft_embed_merge_kernel -- one wave per row --
// rescales to the common maximum and adds in slot order: bit-identical call after call.
//
// GENERIC FORM (any E the dense layer takes, any D >= 1): per chunk of rows (<= 64 MiB of logits) the dense layer writes the logits
// into the workspace (row pitch N rounded up to 4), softmax_rows_kernel -- one wave per row -- turns them into probabilities in
// place (padding columns: zeros) and writes lse, and the dense layer is called again with values^T (transposed once per call into the
// workspace, zero-padded to the same pitch).  The same tail is tal_soft_embed_rows.
#include <math.h>

#include "common.h"
#include "head_plan.h"

namespace tal {

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int NDB> struct VFrag;
template <> struct VFrag<4> { typedef f32x4 type; };
template <> struct VFrag<2> { typedef f32x2 type; };

// E == D.  SEP: values is a matrix of its own (a second LDS image); else values == W and the W image serves both products.
template <int E, bool SEP>
__global__ __launch_bounds__(256, 1) void soft_embed_kernel(const float* __restrict__ feat, int64_t ldf, const float* __restrict__ W,
                                                           const float* __restrict__ bias, const float* __restrict__ V, int64_t M,
                                                           int S, int NT, int64_t U, float* __restrict__ part, int HP) {
    constexpr int GR = E / 4;                 // 16-byte granules per row
    constexpr int NI = SBN * GR / 256;        // granules a thread moves per tile and matrix
    constexpr int NDB = E / 32;               // 32-column blocks of the output
    typedef typename VFrag<NDB>::type vfrag;
    __shared__ __attribute__((aligned(16))) float wbuf[2 * SBN * E];
    __shared__ __attribute__((aligned(16))) float vbuf[SEP ? 2 * SBN * E : 4];
    __shared__ __attribute__((aligned(16))) float bbuf[2 * SBN];
    const int64_t G = gridDim.x;
    const int64_t u0 = (int64_t)blockIdx.x * U / G, u1 = ((int64_t)blockIdx.x + 1) * U / G;
    if (u0 >= u1) return;
    const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
    const int frow = lane & 31, fhalf = lane >> 5;

    // tile n: rows [64 n, 64 n + 64) of W (and of values): thread t moves granule t % GR of rows t / GR + (256 / GR) i, i < NI;
    // rows past S are zeros (their P is exp(-inf) = 0: the bias image holds -inf there)
    const int srow = tid / GR, scol = tid % GR;
    f32x4 prew[NI], prev[SEP ? NI : 1];
    float preb = 0.f;
    auto fetch = [&](int n) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int col = n * SBN + srow + (256 / GR) * i;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            prew[i] = col < S ? *reinterpret_cast<const f32x4*>(W + (int64_t)col * E + scol * 4) : zero;
            if (SEP) prev[i] = col < S ? *reinterpret_cast<const f32x4*>(V + (int64_t)col * E + scol * 4) : zero;
        }
        if (tid < SBN) {
            const int col = n * SBN + tid;
            preb = col < S ? (bias ? bias[col] : 0.f) : -INFINITY;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int row = srow + (256 / GR) * i;
            const int dst = buf * (SBN * E) + row * E + ((scol ^ (row & 15)) * 4);
            *reinterpret_cast<f32x4*>(wbuf + dst) = prew[i];
            if (SEP) *reinterpret_cast<f32x4*>(vbuf + dst) = prev[i];
        }
        if (tid < SBN) bbuf[buf * SBN + tid] = preb;
    };

    f32x4 a[E / 8];           // this wave's 32 x E strip: a[kk] = feat[query, 8 kk + 4 (lane >> 5) .. + 3]
    f32x16 oacc[NDB];         // out^T: element e of block db = out[query][NDB * ((e & 3) + 8 (e >> 2) + 4 (lane >> 5)) + db]
    float mx = -INFINITY, sm = 0.f;       // running maximum of the query; this lane half's share of the running sum
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[db][e] = 0.f;

    fetch((int)(u0 % NT));
    stash(0);
    for (int64_t u = u0; u < u1; ++u) {
        const int64_t m = u / NT;
        const int n = (int)(u - m * NT);
        const int64_t row0 = m * SBM + w * 32;
        const int buf = (int)((u - u0) & 1);
        if (u == u0 || n == 0) {
            int64_t r = row0 + frow;
            r = r < M ? r : M - 1;
            const float* ap = feat + r * ldf + 4 * fhalf;
#pragma unroll
            for (int kk = 0; kk < E / 8; ++kk) a[kk] = *reinterpret_cast<const f32x4*>(ap + 8 * kk);
#pragma unroll
            for (int db = 0; db < NDB; ++db)
#pragma unroll
                for (int e = 0; e < 16; ++e) oacc[db][e] = 0.f;
            mx = -INFINITY;
            sm = 0.f;
        }
        __syncthreads();      // tile u is in LDS (written before this barrier); everyone is done with the other buffer
        const bool more = u + 1 < u1;
        if (more) fetch((int)((u + 1) % NT));
        const float* wb = wbuf + buf * (SBN * E);
        const float* vb = SEP ? vbuf + buf * (SBN * E) : wb;
        const float* bb = bbuf + buf * SBN;

        // scores, transposed: sc[j][e] = z[query = lane & 31][key = 32 j + (e & 3) + 8 (e >> 2) + 4 (lane >> 5)]
        f32x16 sc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) sc[j][e] = 0.f;
#pragma unroll
        for (int kk = 0; kk < E / 8; ++kk) {
            const int sl = ((2 * kk + fhalf) ^ (frow & 15)) * 4;
            f32x4 wf[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) wf[j] = *reinterpret_cast<const f32x4*>(wb + (32 * j + frow) * E + sl);
            const f32x4 fa = a[kk];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                sc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[j].x, fa.x, sc[j], 0, 0, 0);
                sc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[j].y, fa.y, sc[j], 0, 0, 0);
                sc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[j].z, fa.z, sc[j], 0, 0, 0);
                sc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[j].w, fa.w, sc[j], 0, 0, 0);
            }
        }
        // + bias (-inf: a masked column, and every column past S), the tile's maximum of this query
        float cm = -INFINITY;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 bf = *reinterpret_cast<const f32x4*>(bb + 32 * j + 8 * q + 4 * fhalf);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    sc[j][4 * q + c] += bf[c];
                    cm = fmaxf(cm, sc[j][4 * q + c]);
                }
            }
        cm = fmaxf(cm, __shfl_xor(cm, 32, 64));
        // ONE rescale per tile, before any P of this tile exists: everything at the old maximum (output accumulators, running sum)
        // is scaled by f exactly once, everything made below is at the new maximum.  (No finite column so far: the reference point
        // is 0, every exp below is exp(-inf) = 0 and the state stays (-inf, 0, 0).  mx == -inf with a finite tile: f = 0 on zeros.)
        const float mnew = fmaxf(mx, cm);
        const float ms = mnew > -INFINITY ? mnew : 0.f;
        const float f = __expf(mx - ms);
        mx = mnew;
        sm *= f;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int e = 0; e < 16; ++e) oacc[db][e] *= f;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                sc[j][e] = __expf(sc[j][e] - ms);
                sm += sc[j][e];
            }
        // out^T[d, query] += values^T[d, key] * P[key, query]: k-step (j, e) contracts the keys of the two lane halves
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int key = 32 * j + (e & 3) + 8 * (e >> 2) + 4 * fhalf;
                const int g = (NDB == 4 ? frow : frow >> 1) ^ (key & 15);
                const vfrag vf = *reinterpret_cast<const vfrag*>(vb + key * E + g * 4 + (NDB == 4 ? 0 : 2 * (frow & 1)));
#pragma unroll
                for (int db = 0; db < NDB; ++db) oacc[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[db], sc[j][e], oacc[db], 0, 0, 0);
            }
        if (more) stash(buf ^ 1);     // (read last in front of this iteration's barrier)

        if (n == NT - 1 || u == u1 - 1) {
            // this workgroup's share of row block m is complete
            const int slot = (int)((int64_t)blockIdx.x - block_of(m * NT, U, G));
            const int64_t row = row0 + frow;
            const float tot = sm + __shfl_xor(sm, 32, 64);
            if (row < M) {
                float* po = part + (row * HP + slot) * (int64_t)(E + SHDR);
                if (fhalf == 0) {
                    const f32x4 hdr = {mx, tot, 0.f, 0.f};
                    *reinterpret_cast<f32x4*>(po) = hdr;
                }
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int ri = (e & 3) + 8 * (e >> 2) + 4 * fhalf;
                    vfrag o;
#pragma unroll
                    for (int db = 0; db < NDB; ++db) o[db] = oacc[db][e];
                    *reinterpret_cast<vfrag*>(po + SHDR + NDB * ri) = o;
                }
            }
        }
    }
}

// one wave per row: the partials of the row's slots rescaled to the common maximum and added in slot order
__global__ __launch_bounds__(256) void soft_embed_merge_kernel(const float* __restrict__ part, int64_t M, int D, int NT, int64_t U,
                                                              int64_t G, int HP, float* __restrict__ out, float* __restrict__ lse) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int64_t m = row / SBM;
    const int P = (int)(block_of(m * NT + NT - 1, U, G) - block_of(m * NT, U, G) + 1);
    const float* pr = part + row * HP * (int64_t)(D + SHDR);
    float g = -INFINITY;
    for (int p = 0; p < P; ++p) g = fmaxf(g, pr[(int64_t)p * (D + SHDR)]);
    float tot = 0.f, o0 = 0.f, o1 = 0.f;      // D <= 128: columns lane and lane + 64
    for (int p = 0; p < P; ++p) {
        const float* pp = pr + (int64_t)p * (D + SHDR);
        const float f = pp[0] > -INFINITY ? expf(pp[0] - g) : 0.f;      // (a share without a finite column: (-inf, 0, zeros))
        tot += pp[1] * f;
        o0 += pp[SHDR + lane] * f;
        if (lane + 64 < D) o1 += pp[SHDR + lane + 64] * f;
    }
    out[row * D + lane] = o0 / tot;
    if (lane + 64 < D) out[row * D + lane + 64] = o1 / tot;
    if (lane == 0 && lse) lse[row] = g + logf(tot);
}

// probabilities of the rows of a materialised matrix, one wave per row: x [M, ldx] -> p [M, ldp] (p may be x), columns [N, ldp) of
// p are zeroed; p = exp(x - max) / sum (an exact 1, 1/2, 1/4 where the row has 1, 2, 4 equal winners far above the rest)
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* x, int64_t ldx, float* p, int64_t ldp, int64_t M, int N,
                                                          float* __restrict__ lse) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* xr = x + row * ldx;
    float* pr = p + row * ldp;
    float mx = -INFINITY;
    for (int i = lane; i < N; i += 64) mx = fmaxf(mx, xr[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    const float ms = mx > -INFINITY ? mx : 0.f;
    float sm = 0.f;
    for (int i = lane; i < N; i += 64) sm += __expf(xr[i] - ms);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sm += __shfl_xor(sm, off, 64);       // (a fixed tree: every lane holds the same sum)
    for (int i = lane; i < (int)ldp; i += 64) pr[i] = i < N ? __expf(xr[i] - ms) / sm : 0.f;
    if (lane == 0 && lse) lse[row] = mx + logf(sm);
}

// vt [D, ldp] = values^T, columns [N, ldp) zero
__global__ __launch_bounds__(256) void transpose_values_kernel(const float* __restrict__ values, int N, int D, int64_t ldp,
                                                              float* __restrict__ vt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)D * ldp) return;
    const int64_t d = i / ldp, s = i - d * ldp;
    vt[i] = s < N ? values[s * D + d] : 0.f;
}

// the fused launch the plan describes
int launch_soft_embed_fused(const HeadLaunch& p, const float* feat, int64_t ldf, int E, const float* w, const float* b, const float* values,
                            bool sep, int64_t M, int S, float* out, float* lse, void* workspace, hipStream_t s) {
    const int NT = p.NT, hp = p.run.hp;
    const int64_t U = p.U, grid = p.run.grid;
    float* part = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + p.off[0]);
    {
        ProfScope prof(PROF_GEMM, 4.0 * (double)M * (double)S * E, s);
#define SOFT_EMBED_LAUNCH(E_, SEP_)                                                                                                  \
    hipLaunchKernelGGL((soft_embed_kernel<E_, SEP_>), dim3((unsigned)grid), dim3(256), 0, s, feat, ldf, w, b, values, M, S, NT, U, part, hp)
        if (E == 64 && sep)
            SOFT_EMBED_LAUNCH(64, true);
        else if (E == 64)
            SOFT_EMBED_LAUNCH(64, false);
        else if (sep)
            SOFT_EMBED_LAUNCH(128, true);
        else
            SOFT_EMBED_LAUNCH(128, false);
#undef SOFT_EMBED_LAUNCH
        TAL_CHECK_LAUNCH("soft_embed");
    }
    ProfScope prof(PROF_OTHER, (double)p.need, s);
    hipLaunchKernelGGL(soft_embed_merge_kernel, dim3((unsigned)cdiv(M, 4)), dim3(256), 0, s, part, M, E, NT, U, grid, hp, out, lse);
    TAL_CHECK_LAUNCH("soft_embed(merge)");
    return TAL_OK;
}

int launch_transpose_values(const float* values, int N, int D, float* vt, hipStream_t s) {
    const int64_t n = (int64_t)D * pitch4(N);
    ProfScope prof(PROF_OTHER, (double)n * 8.0, s);
    hipLaunchKernelGGL(transpose_values_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, values, N, D, pitch4(N), vt);
    TAL_CHECK_LAUNCH("soft_embed(values^T)");
    return TAL_OK;
}

// rows of probabilities (x -> p, p may be x) and their product with values^T [D, pitch4(N)]
int launch_softmax_matmul(const float* x, int64_t ldx, float* p, int64_t rows, int N, const float* vt, int D, float* out, float* lse,
                          hipStream_t s) {
    const int64_t ldp = pitch4(N);
    {
        ProfScope prof(PROF_OTHER, (double)rows * N * 8.0, s);
        hipLaunchKernelGGL(softmax_rows_kernel, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, s, x, ldx, p, ldp, rows, N, lse);
        TAL_CHECK_LAUNCH("soft_embed(softmax rows)");
    }
    GemmArgs g = {};
    g.A = p; g.W = vt; g.Y = out; g.M = rows; g.N = D; g.K = (int)ldp;
    g.lda = ldp; g.ldw = ldp; g.ldy = D; g.ldres = D; g.nb2 = 1;
    return launch_gemm(g, 0, 1, s);
}

// The entries behind their argument checks (values != NULL): the head on the rows of h [M, ldh] of width E, or on their projection
// (proj_t != NULL); tal_soft_embed_rows: h = the caller's logits [M, N], no w.  The planned call: the fused launch, or values^T once
// and then per chunk of rows (as many at a time as the workspace holds, 64 MiB worth at most) the logits through the dense layer (the
// features' row pitch, the probabilities' padded pitch), probabilities in place -- tal_soft_embed_rows: from the caller's rows --
// and the dense layer again.
int soft_embed(int entry, const float* h, int64_t M, int64_t ldh, int E, const float* proj_t, int E0, const float* w, const float* bias, int N,
               const float* values, int D, float* out, float* lse, void* workspace, size_t workspace_bytes, hipStream_t s) {
    return head_on_rows(
        entry, h, M, ldh, E, proj_t, E0, workspace, workspace_bytes, s,
        [&](const float* feat, int64_t ldf, int width, int proj_in, const void* ws, size_t ws_bytes) {
            return head_call(entry, M, N, width, D, 1, ldf, proj_in, feat, w, values, ws, ws_bytes);
        },
        [&](const HeadCall& c, const HeadLaunch& p, const float* feat, void* ws) {
            if (p.fused) return launch_soft_embed_fused(p, feat, c.ldf, c.E, w, bias, values, c.sep, M, N, out, lse, ws, s);
            float* vt = reinterpret_cast<float*>(ws);
            float* probs = vt + p.vt / 4;
            const bool have_logits = entry == HE_SOFT_EMBED_ROWS;
            const int rc = launch_transpose_values(values, N, D, vt, s);
            return rc ? rc : for_row_chunks(M, p.chunk, [&](int64_t r0, int64_t rows) {
                const float* x = feat + r0 * c.ldf;
                const int rcl = have_logits ? TAL_OK : launch_linear_ld(x, c.ldf, w, bias, rows, N, c.E, probs, p.pitch, s);
                return rcl ? rcl
                           : launch_softmax_matmul(have_logits ? x : probs, have_logits ? c.ldf : p.pitch, probs, rows, N, vt, D, out + r0 * D,
                                                   lse ? lse + r0 : nullptr, s);
            });
        });
}

}  // namespace

}  // namespace tal

using namespace tal;

extern "C" size_t tal_soft_embed_workspace_bytes(int64_t M, int N, int E, int D) {
    return head_query_bytes(head_call(HE_SOFT_EMBED, M, N, E, D, 1, E));
}

extern "C" int tal_soft_embed_fwd(const float* feat, int64_t M, int64_t ldf, int E, const float* w, const float* bias, int N,
                                  const float* values, int D, float* out, float* lse, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    TAL_CHECK_ARG(M >= 0 && E > 0 && N > 0 && D > 0 && ldf >= E, "tal_soft_embed_fwd: bad shape (M=%lld, ldf=%lld, E=%d, N=%d, D=%d)",
                  (long long)M, (long long)ldf, E, N, D);
    TAL_CHECK_ARG(values || D == E, "tal_soft_embed_fwd: values == NULL (values = w) needs D == E (E=%d, D=%d)", E, D);
    if (M == 0) return TAL_OK;
    TAL_CHECK_ARG(feat && w && out, "tal_soft_embed_fwd: null pointer");
    return soft_embed(HE_SOFT_EMBED, feat, M, ldf, E, nullptr, 0, w, bias, N, values ? values : w, D, out, lse, workspace, workspace_bytes,
                      (hipStream_t)stream);
}

extern "C" size_t tal_soft_embed_rows_workspace_bytes(int64_t M, int N, int D) {
    return head_query_bytes(head_call(HE_SOFT_EMBED_ROWS, M, N, D, D, 1, N));
}

extern "C" int tal_soft_embed_rows(const float* x, int64_t M, int N, const float* values, int D, float* out, float* lse,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    TAL_CHECK_ARG(M >= 0 && N > 0 && D > 0, "tal_soft_embed_rows: bad shape (M=%lld, N=%d, D=%d)", (long long)M, N, D);
    if (M == 0) return TAL_OK;
    TAL_CHECK_ARG(x && values && out, "tal_soft_embed_rows: null pointer");
    return soft_embed(HE_SOFT_EMBED_ROWS, x, M, N, D, nullptr, 0, nullptr, nullptr, N, values, D, out, lse, workspace, workspace_bytes,
                      (hipStream_t)stream);
}

extern "C" size_t tal_lm_soft_embed_workspace_bytes(int64_t M, int D, int E0, int V, int col_begin) {
    if (D <= 0 || V <= 0 || col_begin < 0 || col_begin >= V) return 0;
    const size_t head = head_query_bytes(head_call(HE_LM_SOFT_EMBED, M, V - col_begin, E0, E0, 1, E0));
    return head ? lm_proj_bytes(M, E0) + head : 0;
}

extern "C" int tal_lm_soft_embed_fwd(const float* h, int64_t M, int64_t ldh, int D, const float* proj_t, int E0, const float* emb, int V,
                                     int col_begin, float* out, float* lse, void* workspace, size_t workspace_bytes, void* stream) {
    TAL_CHECK_ARG(M >= 0 && D > 0 && E0 > 0 && V > 0 && ldh >= D && ldh % 4 == 0, "tal_lm_soft_embed_fwd: bad shape");
    TAL_CHECK_ARG(col_begin >= 0 && col_begin < V, "tal_lm_soft_embed_fwd: col_begin=%d outside [0, V=%d)", col_begin, V);
    TAL_CHECK_ARG(proj_t || D == E0, "tal_lm_soft_embed_fwd: no projection needs D == E0");
    if (M == 0) return TAL_OK;
    TAL_CHECK_ARG(h && emb && out, "tal_lm_soft_embed_fwd: null pointer");
    const float* keys = emb + (int64_t)col_begin * E0;
    return soft_embed(HE_LM_SOFT_EMBED, h, M, ldh, D, proj_t, E0, keys, nullptr, V - col_begin, keys, E0, out, lse, workspace, workspace_bytes,
                      (hipStream_t)stream);
}
