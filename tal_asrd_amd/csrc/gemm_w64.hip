// The fp16x3 dense layer with ONE wave per SIMD and the whole 512-register file: workgroup tile 256 x 160 x 32,
// 4 waves x (64 rows x 160 columns).  The TDS block's 1x1 Conv1d pair (tal/asr/models.py:312-318,330) on long inputs.
//
// Why: in the 128 x 160 kernel (gemm_f32.hip) a wave owns 32 x 160 and re-reads the whole W tile for 960 cycles of MFMAs --
// 24 fragment reads + 9 LDS-DMA loads per K step.  Here 64 rows share every W fragment: 28 reads + 13 loads per 1,920
// cycles of MFMAs, 28 % fewer operand bytes through L2 -> LDS, and W is re-read by half as many tiles.  What the K loop is
// bound by is the clock the chip sustains under this load, and that depends on the MFMA shape: measured stand-alone
// (scripts/ubench/gemm_f16x3_w64.hip with and without -DMFMA16, profiles/dense_mfma_shape.txt) the loop on 120
// v_mfma_f32_16x16x32_f16 per K step holds 1.51-1.70 GHz at 2,440-2,670 shader cycles per K step, the same loop on 60
// v_mfma_f32_32x32x16_f16 1.35-1.44 GHz at 2,260-2,380 (1,920 is pure MFMA issue in both): 4-6 % more TFLOP/s by wall on
// random data at every TDS width.  DESIGN.md sections 3 and 5.
//
// Structure:
//   * three LDS operand buffers (3 x 52 KB): tile kt + 2 is in flight while tile kt is multiplied; ONE barrier per K step,
//     placed two stages before the step's end, so that the first fragments of tile kt + 1 are read under the last MFMAs
//     of tile kt (one wave per SIMD: nothing else hides an LDS round trip); counted vmcnt, raw s_barrier;
//   * LDS-DMA in inline asm: hipcc would make every ds_read wait for ALL LDS-DMA loads in flight (it cannot tell the
//     buffers apart), which serialises the pipeline; M0 is written in the same statement; completion is counted by hand;
//   * a tile index past the end of K becomes a descriptor with num_records = 0 (the load is dropped by the range check
//     but still counts in vmcnt), so the loop has no tail variants -- hipcc answers multi-exit loops with thousands of
//     spilled registers here;
//   * 80 accumulators of 4 registers (4 row blocks x 10 column blocks of 16 x 16, hi*hi and cross terms): 320 registers, more
//     than the 256 AGPRs.  Every MFMA is inline asm with its accumulator tied in place: 60 in AGPRs ("+a"), row block 3 in
//     VGPRs ("+v").  (Through the builtin hipcc is free to put a 16x16 accumulator in either class and answered this loop
//     with hundreds of AGPR <-> VGPR copies per pass and spills.)  An accumulate chain needs no wait states, and the
//     compiler waits for the ds_reads that feed an asm statement like for any other consumer;
//   * the A fragments (8 per K step) are in use during every stage of a step, so the next step's are read into a second
//     set during the last two stages; three operand buffers x two fragment sets: the K loop is unrolled by six;
//   * same operand geometry, swizzle, arithmetic order per accumulator and epilogues as the 128 x 160 kernel: whole tiles
//     produce bit-identical results.
// The tiles of the last partial scheduling round (1 workgroup per CU: rounds of 256 tiles) are cut along K into slices
// dispatched behind the whole tiles; gemm_splitk_fixup_kernel adds them in a fixed order (as in gemm_f32.hip).
#include <type_traits>

#include "gemm_common.h"

namespace tal {

namespace {

typedef unsigned u32x4w __attribute__((ext_vector_type(4)));

constexpr int W_BM = 256, W_NSUB = 5, W_BN = 32 * W_NSUB, W_ROWS = W_BM + W_BN, W_NBUF = 3;
constexpr int W_CHUNKS = W_ROWS / 8, W_PER_WAVE = W_CHUNKS / 4, W_AT = W_BM / 8 / 4;   // chunk i = w + 4 t; t < W_AT: A rows
constexpr int W_BUF_FLOATS = W_ROWS * 32;
static_assert(W_CHUNKS % 4 == 0, "chunks divide over the waves");

// which LDS-DMA piece (0..12, -1 = none) of tile kt + 2 is issued after MFMA pair `slot` (0..2) of stage q: two per stage,
// stages 0..6 -- all of them before the barrier of stage 8 (evenly spread or three per stage measured the same or worse)
constexpr int dma_piece(int q, int slot) { return (slot < 2 && q < 6) ? 2 * q + slot : (q == 6 && slot == 0) ? 12 : -1; }

// a wave's 64 x 160 tile as 4 row blocks x 10 column blocks of v_mfma_f32_16x16x32_f16 (one MFMA = the whole 32-deep K block)
constexpr int W_RB = 4, W_CB = 2 * W_NSUB;

__device__ __forceinline__ void mfma_vgpr(f32x4& c, const f16x8& a, const f16x8& b) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma_agpr(f32x4& c, const f16x8& a, const f16x8& b) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}
#define W64_MFMA(c, a, b, in_vgpr) do { if (in_vgpr) mfma_vgpr(c, a, b); else mfma_agpr(c, a, b); } while (0)

struct Frags {
    f16x8 ahi[2][W_RB], alo[2][W_RB];     // [fragment set][row block]
    f16x8 bhi[5], blo[5];                 // ring slot = column block % 5
};

}  // namespace

template <int MODE, bool SPLITK, int EPI>
__global__ __launch_bounds__(256, 1) void gemm_w64_kernel(const GemmArgs g) {
    constexpr int NSUB = W_NSUB, RB = W_RB, CB = W_CB, BM = W_BM, BN = W_BN, PER_WAVE = W_PER_WAVE, A_T = W_AT, BUF_FLOATS = W_BUF_FLOATS;
    __shared__ __attribute__((aligned(16))) float lds[W_NBUF * W_BUF_FLOATS];      // 159,744 B: one workgroup per CU

    if (g.stagger_ticks > 0 && blockIdx.x < (unsigned)g.stagger_blocks && (blockIdx.x & 1u)) {
        // (every tile of a round runs the same K loop, so all 256 workgroups reach their epilogue -- a 42 MB write burst with the
        //  matrix pipes idle -- together; a late start of every other first-round workgroup puts the two halves of the chip out
        //  of phase for the whole launch: later workgroups start as CUs free up)
        const unsigned long long t0 = wall_clock64();
        while (wall_clock64() - t0 < (unsigned long long)g.stagger_ticks) __builtin_amdgcn_s_sleep(64);
    }
    // XCD-remapped tile index; SPLITK launches carry the whole-round tiles and, behind them, the K slices of the rest
    const bool is_slice = SPLITK && blockIdx.x >= (unsigned)g.tile_base;
    const unsigned sbid = blockIdx.x - (unsigned)g.tile_base;
    const int slice = is_slice ? (int)(sbid / (unsigned)g.tail_tiles) : 0;
    const unsigned logical = is_slice ? (unsigned)g.tile_base + sbid % (unsigned)g.tail_tiles
                                      : (SPLITK ? logical_tile_of((unsigned)g.tile_base, blockIdx.x) : logical_tile());
    const unsigned tile_m = g.tiles_n == 1 ? logical : __umulhi(logical, g.tiles_n_magic);
    const int64_t m0 = (int64_t)tile_m * BM;
    const int n0 = (int)(logical - tile_m * (unsigned)g.tiles_n) * BN;
    const int64_t M = g.M;
    const int N = g.N, K = g.K;
    const float* A = g.A;
    const float* W = g.W;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = wave_id();

    // operand loads: as in gemm_glds_kernel -- chunk = 8 rows x 128 B, slot s of row r holds the row's logical 16-byte column
    // s ^ ((r >> 1) & 7) (swizzle on the SOURCE address, linear LDS destination)
    const int sub = lane >> 3, srccol = ((lane & 7) ^ (((w & 1) * 4 + (lane >> 4)) & 7)) * 4;
    const int a_rows = (int)((M - m0) < BM ? (M - m0) : BM) - 1;
    const int b_rows = ((N - n0) < BN ? (N - n0) : BN) - 1;
    auto make_rsrc = [](const float* p) {      // buffer descriptor as four SGPR dwords: base, base high (stride 0), num_records, flags
        const uint64_t v = reinterpret_cast<uint64_t>(p);
        u32x4w r;
        r[0] = __builtin_amdgcn_readfirstlane((uint32_t)v);
        r[1] = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
        r[2] = 0x7fffffffu;
        r[3] = 0x00020000u;
        return r;
    };
    const u32x4w rs_a = make_rsrc(A + m0 * g.lda), rs_w = make_rsrc(W + (int64_t)n0 * g.ldw);
    const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) float*)lds) + (unsigned)w * 1024u;
    int voff[PER_WAVE];
#pragma unroll
    for (int t = 0; t < PER_WAVE; ++t) {
        const int row = 8 * (w + 4 * t) + sub;
        voff[t] = t < A_T ? (int)((min(row, a_rows) * g.lda + srccol) * 4) : (int)((min(row - BM, b_rows) * g.ldw + srccol) * 4);
    }
    auto dma = [&](int t, unsigned nrec, int bufoff, int kofs) {
        const unsigned dst = lds_base + (unsigned)(bufoff * 4 + t * 4096);
        u32x4w rs = t < A_T ? rs_a : rs_w;
        rs[2] = nrec;
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(dst), "v"(voff[t]), "s"(rs), "s"(kofs) : "memory");
    };

    // accumulators: hh = sum hi*hi (EPI: started from the bias), xx = the cross terms hi*lo + lo*hi (scaled by 2^11).
    // C/D layout of the 16x16 MFMA with the activations as its A operand: col = lane & 15, row = 4*(lane>>4) + e -- all four
    // elements of an accumulator belong to one column.
    f32x4 hh[RB][CB], xx[RB][CB];
#pragma unroll
    for (int j = 0; j < CB; ++j) {
        const float b0 = (EPI && g.bias && !is_slice) ? g.bias[n0 + j * 16 + (lane & 15)] : 0.f;
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                hh[i][j][e] = b0;
                xx[i][j][e] = 0.f;
            }
    }

    // fragment addresses: row (lane & 15) of a 16-row block; logical 16-byte slot fq (hi halves) / 4 + fq (lo halves) sits at
    // physical slot logical ^ fsw.  The four hi slots of a row's 128-byte K block are the four k groups of one MFMA.
    const int frow = lane & 15, fsw = (frow >> 1) & 7, fq = lane >> 4;
    const int a_lane = (w * 64 + frow) * 32, b_lane = (BM + frow) * 32;
    const int sh = (fq ^ fsw) * 4, sl = ((4 + fq) ^ fsw) * 4;
    Frags f;
    auto read_ahi = [&](int set, int bufoff) {
#pragma unroll
        for (int i = 0; i < RB; ++i) f.ahi[set][i] = *reinterpret_cast<const f16x8*>(lds + bufoff + a_lane + i * 16 * 32 + sh);
    };
    auto read_alo = [&](int set, int bufoff) {
#pragma unroll
        for (int i = 0; i < RB; ++i) f.alo[set][i] = *reinterpret_cast<const f16x8*>(lds + bufoff + a_lane + i * 16 * 32 + sl);
    };
    auto rb = [&](int j, int bufoff) {          // W fragments of column block j into ring slot j % 5
        f.bhi[j % 5] = *reinterpret_cast<const f16x8*>(lds + bufoff + b_lane + j * 16 * 32 + sh);
        f.blo[j % 5] = *reinterpret_cast<const f16x8*>(lds + bufoff + b_lane + j * 16 * 32 + sl);
    };

    const int nk_all = K / BK;
    const int kt0 = is_slice ? (int)((int64_t)slice * nk_all / g.split) : 0;
    const int kt1 = is_slice ? (int)((int64_t)(slice + 1) * nk_all / g.split) : nk_all;
    constexpr unsigned NREC = 0x7fffffffu;
    // prologue: tiles kt0 and kt0 + 1 in flight, tile kt0 landed, first fragments read
#pragma unroll
    for (int t = 0; t < PER_WAVE; ++t) dma(t, NREC, 0, kt0 * (BK * 4));
    {
        const unsigned nrec = kt0 + 1 < kt1 ? NREC : 0u;
#pragma unroll
        for (int t = 0; t < PER_WAVE; ++t) dma(t, nrec, BUF_FLOATS, (kt0 + 1) * (BK * 4));
    }
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER_WAVE) : "memory");
    __builtin_amdgcn_s_barrier();
    read_ahi(0, 0);
    rb(0, 0);
    rb(1, 0);
    read_alo(0, 0);
    // one K step on the tile in buffer BUFC with the A fragments of set SETC.  A stage is one column block: its W fragment pair
    // serves four MFMA triples, row blocks innermost (no two consecutive MFMAs write the same accumulator).  Per accumulator
    // element and K block: hh += a_hi.b_hi, xx += a_hi.b_lo, xx += a_lo.b_hi.  The A fragments are in use during every stage,
    // so the next step's go into the other set (stages 8, 9).  The loop is unrolled by six (three operand buffers x two
    // fragment sets) so that every LDS address is a lane constant + an immediate and every register a fixed one (a rotating
    // run-time offset also makes hipcc lose the 16-byte alignment of the fragment reads).
    auto step = [&](auto bufc, auto setc, int kt) {
        constexpr int cur = decltype(bufc)::value * BUF_FLOATS, nxt = ((decltype(bufc)::value + 1) % 3) * BUF_FLOATS,
                      fil = ((decltype(bufc)::value + 2) % 3) * BUF_FLOATS, set = decltype(setc)::value;
        const int kofs = (kt + 2) * (BK * 4);
        const unsigned nrec = kt + 2 < kt1 ? NREC : 0u;
#pragma unroll
        for (int q = 0; q < CB; ++q) {
            const int s = q % 5;
            if (q == 8) {
                // tile kt + 1 has landed (this wave's share: all but the 13 youngest loads) and is visible to all waves
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER_WAVE) : "memory");
                __builtin_amdgcn_s_barrier();
            }
            if (q + 2 < CB) rb(q + 2, cur);
            else rb(q + 2 - CB, nxt);                     // stages 0 / 1 of the next step
            if (q == 8) read_ahi(set ^ 1, nxt);
            if (q == 9) read_alo(set ^ 1, nxt);
            __builtin_amdgcn_sched_barrier(0);
            // 20 of the 80 accumulators live in VGPRs: row block 3
#pragma unroll
            for (int i = 0; i < RB; ++i) W64_MFMA(hh[i][q], f.ahi[set][i], f.bhi[s], i == RB - 1);
            if (dma_piece(q, 0) >= 0) { __builtin_amdgcn_sched_barrier(0); dma(dma_piece(q, 0), nrec, fil, kofs); __builtin_amdgcn_sched_barrier(0); }
#pragma unroll
            for (int i = 0; i < RB; ++i) W64_MFMA(xx[i][q], f.ahi[set][i], f.blo[s], i == RB - 1);
            if (dma_piece(q, 1) >= 0) { __builtin_amdgcn_sched_barrier(0); dma(dma_piece(q, 1), nrec, fil, kofs); __builtin_amdgcn_sched_barrier(0); }
#pragma unroll
            for (int i = 0; i < RB; ++i) W64_MFMA(xx[i][q], f.alo[set][i], f.bhi[s], i == RB - 1);
            if (dma_piece(q, 2) >= 0) { __builtin_amdgcn_sched_barrier(0); dma(dma_piece(q, 2), nrec, fil, kofs); }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    int kt = kt0;
    for (; kt + 6 <= kt1; kt += 6) {
        step(I0(), I0(), kt);
        step(I1(), I1(), kt + 1);
        step(I2(), I0(), kt + 2);
        step(I0(), I1(), kt + 3);
        step(I1(), I0(), kt + 4);
        step(I2(), I1(), kt + 5);
    }
    if (kt < kt1) step(I0(), I0(), kt);
    if (kt + 1 < kt1) step(I1(), I1(), kt + 1);
    if (kt + 2 < kt1) step(I2(), I0(), kt + 2);
    if (kt + 3 < kt1) step(I0(), I1(), kt + 3);
    if (kt + 4 < kt1) step(I1(), I0(), kt + 4);
    // every LDS-DMA has landed (dropped ones included) and the last MFMA results are readable; then all waves are done with
    // the operand buffers before they become the store stage
    asm volatile("s_waitcnt vmcnt(0)\n\ts_nop 15\n\ts_nop 15" ::: "memory");
    __syncthreads();

    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 s11 = {1.0f / 2048.0f, 1.0f / 2048.0f};
    // (a lambda called twice with a compile-time row block: the generic epilogue is too large for hipcc to unroll a loop around
    //  it, and a run-time index would send the accumulators to scratch memory for the whole kernel)
    auto finish = [&](auto bc) {
        constexpr int b = decltype(bc)::value;          // 32 rows = row blocks 2 b, 2 b + 1
        f32x4 acc[2][CB];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < CB; ++j)
#pragma unroll
                for (int e = 0; e < 4; e += 2) {
                    const f32x2 x2 = {xx[2 * b + i][j][e], xx[2 * b + i][j][e + 1]}, a2 = {hh[2 * b + i][j][e], hh[2 * b + i][j][e + 1]};
                    const f32x2 o2 = __builtin_elementwise_fma(x2, s11, a2);
                    acc[i][j][e] = o2[0];
                    acc[i][j][e + 1] = o2[1];
                }
        // the shared epilogues address rows as m0 + 32 w + ...: this wave's row block b starts at m0 + 64 w + 32 b
        const int64_t m0e = m0 + 32 * w + 32 * b;
        if (b == 1) __builtin_amdgcn_wave_barrier();        // (the wave's stage slice is reused: LDS operations of a wave are in order)
        if (is_slice) {
            GemmArgs gp = g;
            gp.M = m0 + BM;
            gp.N = n0 + BN;
            gp.ldy = BN;
            gp.out_split = 0;            // partial sums stay fp32; the fix-up kernel writes the split form
            float* tile_ws = g.splitk_ws + ((size_t)(logical - g.tile_base) * g.split + slice) * (BM * BN);
            gemm_epilogue<0, NSUB, true>(gp, acc, lds, tile_ws - (m0 * BN + n0), nullptr, nullptr, m0e, n0, lane, w, w, 0);
        } else {
            if constexpr (EPI != 0) gemm_epilogue_split<MODE, NSUB, true>(g, acc, lds, g.Y, g.res, m0e, n0, lane, w);
            else gemm_epilogue<MODE, NSUB, true>(g, acc, lds, g.Y, g.bias, g.res, m0e, n0, lane, w, w, 0);
        }
    };
    finish(std::integral_constant<int, 0>());
    finish(std::integral_constant<int, 1>());
}

// the step's kernel: K-sliced tail or whole tiles only, static-addressing split epilogue (modes 1 / 2: E) or the shared one
void launch_gemm_w64(const GemmArgs& g, int mode, const GemmStep& st, hipStream_t s) {
    const dim3 grid(st.grid_x), b(256);
    with_mode(mode, [&](auto m) {
        constexpr int MODE = decltype(m)::value, E = MODE == 1 || MODE == 2;
        if constexpr (MODE <= 3) {
            if (st.splitk && st.epi) hipLaunchKernelGGL((gemm_w64_kernel<MODE, true, E>), grid, b, 0, s, g);
            else if (st.splitk) hipLaunchKernelGGL((gemm_w64_kernel<MODE, true, 0>), grid, b, 0, s, g);
            else if (st.epi) hipLaunchKernelGGL((gemm_w64_kernel<MODE, false, E>), grid, b, 0, s, g);
            else hipLaunchKernelGGL((gemm_w64_kernel<MODE, false, 0>), grid, b, 0, s, g);
        }
    });
}

}  // namespace tal
