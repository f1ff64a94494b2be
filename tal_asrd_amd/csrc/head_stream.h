// The streaming head: something per row of z[r, s] = feat[r, :] . W[s, :] + b[s] next to the row's log-sum-exp, without the logits
// in memory.  ONE kernel, head_stream_kernel<E, Scan>; what is kept per row is the Scan policy's business (csrc/head_topk.hip: a
// sorted top-k list; csrc/xent.hip: the arg-max and the target's logit).
//
// Each wave keeps its 32 x E feature strip as E / 8 MFMA-ready fragments, W streams through LDS in 128-column N tiles (double-
// buffered 128 x 32 chunks in the dense layers' XOR-swizzled image, one barrier per chunk), the products are v_mfma_f32_32x32x2_f32
// (exact fp32), work is cut into equal runs of (row block, N tile) units (csrc/head_plan.h).
//   * W is staged with ordinary global loads into registers (issued under the MFMAs of the chunk before) and LDS writes -- no
//     LDS-DMA, so there is no load in flight at a barrier that the compiler does not wait for by itself.
//   * Per-row state per accumulator element would take 16 rows x state registers per lane.  Instead, after an N tile's MFMAs the
//     wave writes its logits (+ bias) to a wave-private LDS tile one 32 x 32 sub-tile at a time (row pitch 33: the 32 lanes of a half
//     wave, which read one column of 32 different rows, hit 32 different banks) and TWO LANES PER ROW scan 16 columns each: block
//     maximum first, ONE rescale of the running (max, sum exp(z - max)) per block, then the exps (LseState), then the policy's visit
//     of the same 16 values.  Register cost: the policy's state + 2, independent of the tile.
// A workgroup leaves, per row, per slot (its rank among the workgroups of that row block) and per lane half, one partial: the
// policy's state and (max, sum).  The policy's merge kernel -- one wave per row, one partial per lane, so 2 x HS_SLOTS <= 64 -- adds
// the sums rescaled to the common maximum in a fixed butterfly order (lse_lanes): bit-identical call after call.
//
// A Scan is a plain struct, every member inlined:
//   Args                       what the policy needs from the launch (by value in the kernel arguments)
//   begin(args, row, M, S)     a row block starts: reset the state of `row` (row >= M: a padding row, nothing of it is kept)
//   block(x, col0, nv)         16 scanned logits, columns [col0, col0 + 16) of which the first nv exist (nv may be <= 0 or > 16)
//   leave(args, base, lse)     write the partial of base = (row * HP + slot) * 2 + lane half
#pragma once
#include <math.h>

#include "common.h"
#include "head_plan.h"

namespace tal {

constexpr int HS_NSUB = 4;           // 32-column sub-tiles of an N tile (HS_BM, HS_BN, HS_SLOTS: csrc/head_plan.h)
constexpr int HS_PITCH = 33;         // row pitch (floats) of a wave's 32 x 32 logit tile
constexpr int NOIDX = 0x7fffffff;

// the order of the results: value descending, index ascending among equal values (-inf columns included; the empty entry
// (-inf, NOIDX) ranks below every column)
__device__ __forceinline__ bool better(float v, int i, float tv, int ti) { return v > tv || (v == tv && i < ti); }

// running (max, sum exp(z - max)) of one lane
struct LseState {
    float mx = -INFINITY, sm = 0.f;
    __device__ __forceinline__ void clear() {
        mx = -INFINITY;
        sm = 0.f;
    }
    __device__ __forceinline__ void block(const float (&x)[16], int nv) {
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
    }
};

// log-sum-exp of a row from one (max, sum) per lane of a wave (empty: (-inf, 0)): the sums rescaled to the common maximum and
// added in a fixed tree, so every lane holds the same value
__device__ __forceinline__ float lse_lanes(float mx, float sm) {
    float g = mx;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) g = fmaxf(g, __shfl_xor(g, off, 64));
    float t = mx > -INFINITY ? sm * expf(mx - g) : 0.f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
    return g + logf(t);
}

template <int E, class Scan>
__global__ __launch_bounds__(256, 2) void head_stream_kernel(const float* __restrict__ feat, int64_t ldf, const float* __restrict__ W,
                                                            const float* __restrict__ bias, int64_t M, int S, int NT, int64_t U,
                                                            const typename Scan::Args args, int HP) {
    __shared__ __attribute__((aligned(16))) float wbuf[2 * HS_BN * 32];    // 32,768 B
    __shared__ float tile[4 * 32 * HS_PITCH];                              // 16,896 B
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
            const int col = n * HS_BN + srow + 32 * i;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            pre[i] = col < S ? *reinterpret_cast<const f32x4*>(W + (int64_t)col * E + kt * 32 + scol * 4) : zero;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(wbuf + buf * (HS_BN * 32) + sdst + i * (32 * 32)) = pre[i];
    };

    f32x4 a[E / 8];           // this wave's 32 x E strip: a[kk] = A[row, 8 kk + 4 (lane >> 5) .. + 3]
    f32x16 acc[HS_NSUB];
#pragma unroll
    for (int j = 0; j < HS_NSUB; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    // scan state of this lane: row (lane & 31) of the wave's strip, columns [16 (lane >> 5), + 16) of every 32-column sub-tile
    LseState lse;
    Scan scan;
    float* mytile = tile + w * (32 * HS_PITCH);

    // (E / 32 is even: the chunk after a unit's last lands in buffer 0, where the next unit's kt = 0 looks for it)
    static_assert((E / 32) % 2 == 0, "the double buffer's parity needs an even number of chunks per unit");
    fetch((int)(u0 % NT), 0);
    stash(0);
    for (int64_t u = u0; u < u1; ++u) {
        const int64_t m = u / NT;
        const int n = (int)(u - m * NT);
        const int64_t row0 = m * HS_BM + w * 32;
        if (u == u0 || n == 0) {
            int64_t r = row0 + frow;
            scan.begin(args, r, M, S);
            r = r < M ? r : M - 1;
            const float* ap = feat + r * ldf + 4 * fhalf;
#pragma unroll
            for (int kk = 0; kk < E / 8; ++kk) a[kk] = *reinterpret_cast<const f32x4*>(ap + 8 * kk);
            lse.clear();
        }
        float bcol[HS_NSUB];
#pragma unroll
        for (int j = 0; j < HS_NSUB; ++j) {
            const int col = n * HS_BN + j * 32 + frow;
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
            const float* Bs = wbuf + buf * (HS_BN * 32) + frow * 32;
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) {
                const int sl = ((2 * k4 + fhalf) ^ fsw) * 4;
                f32x4 fb[HS_NSUB];
#pragma unroll
                for (int j = 0; j < HS_NSUB; ++j) fb[j] = *reinterpret_cast<const f32x4*>(Bs + j * 32 * 32 + sl);
                const f32x4 fa = a[kt * 4 + k4];
#pragma unroll
                for (int j = 0; j < HS_NSUB; ++j) {
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
        for (int j = 0; j < HS_NSUB; ++j) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                mytile[((e & 3) + 8 * (e >> 2) + 4 * fhalf) * HS_PITCH + frow] = acc[j][e] + bcol[j];
                acc[j][e] = 0.f;
            }
            // the tile is this wave's own: its LDS instructions execute in order, the fences keep the compiler from reordering them
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int col0 = n * HS_BN + j * 32 + fhalf * 16;
            float x[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) x[c] = mytile[frow * HS_PITCH + fhalf * 16 + c];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int nv = S - col0;          // columns [col0, col0 + nv) exist
            lse.block(x, nv);
            scan.block(x, col0, nv);
        }
        if (n == NT - 1 || u == u1 - 1) {
            // this workgroup's share of row block m is complete
            const int slot = (int)((int64_t)blockIdx.x - block_of(m * NT, U, G));
            const int64_t row = row0 + frow;
            if (row < M) scan.leave(args, (row * HP + slot) * 2 + fhalf, lse);
        }
    }
}

}  // namespace tal
