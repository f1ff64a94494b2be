// What launch_gemm (csrc/gemm_f32.hip) launches for a dense layer: kernel family, template choices, grid, tile geometry and the
// K-sliced tail, decided from the call's shape, flags, address alignment, scratch size, CU count and options alone.  Plain C++ (no
// HIP types, no pointer dereferenced, no heap; the plan comes back by value), so that tests/test_gemm_plan_cpu.py can walk every
// arm with a host compiler.  launch_gemm checks its arguments, asks for the plan and launches the steps in order.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace tal {

// the dense-layer switches of tal_set_option, read once per call
struct GemmOpts {
    int s64_below, no_w64, no_glds, no_splitk4, no_splitk_tail, no_row_split, no_n96, global_loads, s64_rows, s64_order, w64_stagger;
};

// The facts of a call the decisions rest on.  *_lo: the low four address bits (a NULL bias / res counts as aligned, which is all
// the decisions ask of it); launch_gemm has checked the arguments, so mode 2 has a residual and the fp16x3 form has K % 32 == 0.
struct GemmCall {
    int64_t M;
    int N, K, mode, nbatch;
    bool f16x3, out_split, res_split;
    int64_t lda, ldw, ldy, ldres;
    bool has_ws, has_range_flag;
    unsigned a_lo, w_lo, y_lo, res_lo, bias_lo;
    size_t splitk_ws_bytes;
    int cus;
    GemmOpts o;
};

enum GemmKernel {
    GK_S64,         // gemm_s64_kernel: 64 x 80 (32 x 80 with two waves) tiles, fp16x3 relu / residual layers of short inputs
    GK_W64,         // gemm_w64_kernel: 256 x 160 tiles, one wave per SIMD, fp16x3
    GK_GLDS,        // gemm_glds_kernel: LDS-DMA 128 x 160 or 128 x 96 tiles
    GK_SPLITK4,     // gemm_splitk4_kernel: 32 x 32 tiles, the four waves split K (M <= 512)
    GK_TILE_K256,   // gemm_nt_f32_kernel<1, 1, 128>: 32 x 128 register tile, M <= 512 and K >= 256
    GK_TILE_SMALL,  // gemm_nt_f32_kernel<1, 1, 32>: 32 x 128 register tile, M <= 512 and K < 256
    GK_TILE_LARGE   // gemm_nt_f32_kernel<4, 5, 32>: 128 x 160 register tile (K % 32 != 0, a misaligned operand, gemm_no_glds)
};

// One ProfScope and one kernel launch (two with fixup_grid > 0: the ordered sum of the K slices follows) over the rows
// [row0, row0 + rows) of the call.  grid_x = tile_base whole tiles + tail_tiles * split K slices when split >= 2, else all tiles.
struct GemmStep {
    int kernel;                     // GemmKernel
    int bm, bn;                     // tile shape
    int nsub, waves, stage, epi;    // GK_GLDS: 32-column blocks per wave (5 / 3), operand loads (2 = buffer form, 0 = global), EPI; GK_S64: waves
    bool splitk;
    unsigned grid_x, grid_y, block, fixup_grid;
    int tiles_n, tiles_m;
    unsigned tiles_n_magic, tiles_m_magic;
    int tile_base, split, tail_tiles, n_major, stagger_ticks, stagger_blocks;
    int64_t row0, rows;
    double work;                    // flops of the step's profiling scope
};

// Steps per call: every row split takes floor(cus / tiles_n) * tiles_n > cus / 2 of the call's fewer than 2 cus 256-row tiles and
// needs cus of them left, so a call splits at most twice: two row blocks and the launch of what remains.
constexpr int GEMM_PLAN_MAX_STEPS = 3;
struct GemmPlan {
    int n;
    bool grid_too_large;            // refused ("gemm: grid too large"): nothing is launched
    GemmStep step[GEMM_PLAN_MAX_STEPS];
};

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// t / d == umulhi(t, magic_of(d)) for every tile index t < nb while nb * d < 2^32 (magic_exact); the kernels skip the multiply at d == 1
inline unsigned magic_of(int d) { return d > 1 ? (unsigned)((1ull << 32) / (unsigned)d) + 1u : 0u; }
inline bool magic_exact(int64_t nb, int d) { return nb * d < (1ll << 32); }

// tal_linear_workspace_bytes: may a dense layer of this shape cut the tiles of its last round along K (LDS-DMA kernels, >= 2 slices
// of >= 4 K steps), i.e. is scratch worth passing
inline bool gemm_wants_scratch(int64_t M, int N, int K) { return M > 512 && K % 32 == 0 && K >= 256 && N > 0; }

// May a launch with `bn`-wide tiles take the static-addressing split epilogue (EPI = 1: the TDS block's relu / residual layers,
// split-form output under the range guard, mode 2 with a split-form residual)?  Its store pattern has no column tail and no batch.
inline bool split_epilogue_ok(const GemmCall& c, int bn, unsigned grid_y) {
    const bool y_ok = c.ldy % 4 == 0 && c.ldy < (1 << 21) && (c.y_lo & 15) == 0 && c.N % bn == 0;
    const bool r_ok = c.mode != 2 || (c.res_split && c.ldres % 4 == 0 && c.ldres < (1 << 21) && (c.res_lo & 15) == 0);
    return c.f16x3 && (c.mode == 1 || c.mode == 2) && c.out_split && c.has_range_flag && y_ok && r_ok && grid_y == 1;
}

// Stream-K-lite: a launch proceeds in rounds of `slots` resident tiles; the `rem` tiles of the last, partial round are cut along K
// into `split` slices each, so that they occupy the whole chip for a fraction of a round instead of part of it for a whole one.  The
// slices are blocks of the same launch, dispatched behind the whole tiles; a fix-up kernel adds them in a fixed order.  Cost of a
// candidate in rounds: the slices' own rounds, ceil(rem * split / slots) / split, + their scratch traffic (each slice writes and
// the fix-up re-reads an fp32 tile of `tile_bytes`, ~4 TB/s) relative to one round's duration round_us; the cheapest within the
// scratch size wins when it beats one more whole round.  Returns 0 (no slices) or 2..8, with >= 4 of the nk K steps per slice.
inline int splitk_tail(int64_t rem, int64_t slots, int nk, size_t tile_bytes, size_t ws_bytes, double round_us) {
    int split = 0;
    double best = 0.97;
    for (int sp = 2; sp <= 8 && sp <= nk / 4; ++sp) {
        if ((size_t)rem * sp * tile_bytes > ws_bytes) break;
        const double traffic_us = (double)rem * sp * (2.0 * tile_bytes) / 4.0e6;
        const double tail = (double)cdiv(rem * sp, slots) / sp + traffic_us / round_us;
        if (tail < best) { best = tail; split = sp; }
    }
    return split;
}

// 128-row LDS-DMA tiles, two workgroups resident per CU: duration of `tiles` tiles in us.  Per K step of a round
// (scripts/bench_gemm_short.py): 0.82 with one workgroup per CU, 1.27 with two, x scale (= NSUB / 5).
inline double glds_rounds_us(int64_t tiles, double scale, int64_t slots, int nk) {
    const int64_t fr = tiles / slots, r = tiles % slots;
    const double two = 10.0 + 1.27 * scale * nk, one = 10.0 + 0.82 * scale * nk;
    return fr * two + (r == 0 ? 0.0 : (r <= slots / 2 ? one : two));
}

inline void plan_tiles(GemmStep& st, int kernel, int bm, int bn, int tiles_n, int64_t grid_x, int nbatch) {
    st.kernel = kernel; st.bm = bm; st.bn = bn;
    st.tiles_n = tiles_n; st.tiles_n_magic = magic_of(tiles_n);
    st.grid_x = (unsigned)grid_x; st.grid_y = (unsigned)nbatch; st.block = 256;
}
// grid = [full whole tiles | split K slices of each of the rem tail tiles]; the fix-up takes 32 rows per workgroup
inline void plan_tail(GemmStep& st, int64_t full, int64_t rem, int split) {
    st.splitk = true;
    st.tile_base = (int)full; st.split = split; st.tail_tiles = (int)rem;
    st.grid_x = (unsigned)(full + rem * split);
    st.fixup_grid = (unsigned)rem * (unsigned)(st.bm / 32);
}
// 256 x 160 launches of at least two rounds: the odd workgroups of the first round start gemm_w64_stagger percent of a tile's
// duration late (one round has nothing to be out of phase with)
inline void plan_w64(GemmStep& st, const GemmCall& c) {
    st.epi = split_epilogue_ok(c, 160, 1);
    if (c.o.w64_stagger > 0 && st.grid_x >= 2u * (unsigned)c.cus) {
        const double tile_us = 1.39 * (c.K / 32) + 12.0;              // scripts/bench_gemm_f16x3_fit.py: K step + fixed cost per round
        st.stagger_ticks = (int)(tile_us * c.o.w64_stagger);          // us * pct / 100 * 100 ticks per us
        st.stagger_blocks = c.cus;
    }
}

// fp16x3 relu / residual layer on 64 x 80 tiles (gemm_s64.hip): whole tiles only, N % 80 == 0, 16-byte operands
inline bool gemm_s64_ok(const GemmCall& c) {
    if (!(c.mode == 1 || c.mode == 2) || !c.f16x3 || c.N % 80 != 0 || c.K % 32 != 0) return false;
    if (((c.a_lo | c.w_lo | c.y_lo | c.bias_lo) & 15) != 0) return false;
    if (c.ldy % 4 != 0 || c.lda >= (1 << 21) || c.ldw >= (1 << 21)) return false;
    if (c.mode == 2 && ((c.res_lo & 15) != 0 || c.ldres % 4 != 0)) return false;
    if ((c.out_split && c.N % 32 != 0) || (c.mode == 2 && c.res_split && c.ldres % 32 != 0)) return false;
    return true;
}

inline GemmPlan gemm_plan(GemmCall c) {
    GemmPlan p = {};
    const GemmOpts& o = c.o;
    const int nk = c.K / 32;
    int64_t row0 = 0;
    for (;;) {      // (only a row split comes back here, with the rows it left)
        GemmStep& st = p.step[p.n++];
        st.row0 = row0;
        st.rows = c.M;
        st.work = 2.0 * (double)c.M * (double)c.N * (double)c.K * c.nbatch;
        const bool aligned16 = ((c.a_lo | c.w_lo) & 15) == 0;
        // short inputs: 64 x 80 tiles, whole tiles only, while they fit one round of two workgroups per CU (measured against the
        // K-sliced launches below: ahead up to 470 / 336 / 432 tiles at N = K = 800 / 1120 / 1440, behind from 590 / 658 / 846,
        // profiles/r3_gemm_short_inputs.txt)
        if (c.f16x3 && c.nbatch == 1 && cdiv(c.M, 64) * (c.N / 80) <= (int64_t)o.s64_below * c.cus && gemm_s64_ok(c)) {
            // 32-row tiles (two waves per workgroup) while even those leave CUs idle: stage 3 of a 30-second clip is 108 tiles of 64
            // rows on 256 CUs, 216 of 32.  gemm_s64_rows: 1 / 2 force 64 / 32 rows.
            const int tiles_n = c.N / 80;
            const bool half = o.s64_rows == 2 || (o.s64_rows == 0 && cdiv(c.M, 32) * tiles_n <= (int64_t)c.cus);
            st.tiles_m = (int)cdiv(c.M, half ? 32 : 64);
            st.tiles_m_magic = magic_of(st.tiles_m);
            plan_tiles(st, GK_S64, half ? 32 : 64, 80, tiles_n, (int64_t)st.tiles_m * tiles_n, 1);
            st.waves = half ? 2 : 4;
            st.block = 64 * st.waves;
            // An XCD (its own L2) takes a contiguous eighth of the tile order.  Fewer rows than columns: W (N x K) is the larger
            // operand, so the order keeps an XCD on a few W panels; otherwise on a few X panels (measured,
            // profiles/r4_gemm_s64_order_depth.txt: 30.5 -> 28.8 us per layer pair at 376 rows x 1440, 28.0 -> 26.6 at 751 x 1120;
            // the other way round it loses as much).  gemm_s64_order: 1 / 2 force m-major / n-major.
            st.n_major = o.s64_order == 1 ? 0 : o.s64_order == 2 ? 1 : (c.M < (int64_t)c.N ? 1 : 0);
            return p;
        }
        // fp16x3 launches with at least one full round of 256 x 160 tiles (one workgroup per CU) take the one-wave-per-SIMD kernel
        // (gemm_w64.hip); the tiles of its last partial round are cut along K like the 128 x 160 kernel's
        if (c.f16x3 && c.nbatch == 1 && !o.no_w64 && !o.no_glds && aligned16) {
            const int64_t slots = c.cus;
            const int tiles_n = (int)cdiv(c.N, 160);
            const int64_t nb = cdiv(c.M, 256) * tiles_n;
            if (nb >= slots && nb < (1ll << 31) && magic_exact(nb, tiles_n)) {
                // ONE full round and a remainder of a few thousand rows (a 5-minute clip's first stage: 295 tiles): the rows of the
                // whole round's row blocks are a step of their own, the rest goes through the decisions again (64 x 80 or 128 x 96 /
                // 160 tiles) -- K slices of the 39 leftover tiles plus their fix-up launch cost 34 us on top of the round's 45, the
                // second launch ~16.  Rows are independent: results do not change.
                const int64_t rb = slots / tiles_n, rows1 = rb * 256;
                if (nb < 2 * slots && nb % slots != 0 && rb >= 1 && c.M - rows1 > 128 && c.M - rows1 <= 4096 && !o.no_row_split &&
                    p.n < GEMM_PLAN_MAX_STEPS) {
                    st.rows = rows1;
                    st.work = 2.0 * (double)rows1 * (double)c.N * (double)c.K;
                    plan_tiles(st, GK_W64, 256, 160, tiles_n, rb * tiles_n, 1);
                    plan_w64(st, c);
                    // the remainder's operands start rows1 rows further on (rows1 is a multiple of 256 rows of 4-byte elements, so
                    // the low address bits come out as they went in; they are derived here, not assumed)
                    row0 += rows1;
                    c.M -= rows1;
                    c.a_lo = (unsigned)((c.a_lo + rows1 * c.lda * 4) & 15);
                    c.y_lo = (unsigned)((c.y_lo + rows1 * c.ldy * 4) & 15);
                    c.res_lo = (unsigned)((c.res_lo + rows1 * c.ldres * 4) & 15);
                    continue;
                }
                plan_tiles(st, GK_W64, 256, 160, tiles_n, nb, 1);
                // round: ~1.5 us per K step + ~12 us per tile, scripts/ubench/gemm_f16x3_w64.hip
                const int64_t rem = nb % slots;
                const int split = rem > 0 && c.has_ws && !o.no_splitk_tail
                                      ? splitk_tail(rem, slots, nk, (size_t)256 * 160 * 4, c.splitk_ws_bytes, 1.5 * nk + 12.0) : 0;
                if (split >= 2) plan_tail(st, nb - rem, rem, split);
                plan_w64(st, c);
                return p;
            }
        }
        const bool small = c.M <= 512 && !c.f16x3;
        const int bm = small ? 32 : 128, bn = small ? 128 : 160;
        const int tiles_n = (int)cdiv(c.N, bn);
        const int64_t nb = cdiv(c.M, bm) * tiles_n;
        p.grid_too_large = !(nb < (1ll << 31) && magic_exact(nb, tiles_n));
        if (p.grid_too_large) return p;
        // small problems are latency-bound (a K step costs one L2 round trip, not its 16 MFMAs): a 128-deep K slab quarters the
        // number of dependent round trips
        if (small && c.mode != 4 && aligned16 && !o.no_splitk4) {
            const int64_t nb32 = cdiv(c.M, 32) * cdiv(c.N, 32);
            p.grid_too_large = !(nb32 < (1ll << 31));
            plan_tiles(st, GK_SPLITK4, 32, 32, (int)cdiv(c.N, 32), nb32, c.nbatch);
        } else if (small) {
            plan_tiles(st, c.K >= 256 ? GK_TILE_K256 : GK_TILE_SMALL, bm, bn, tiles_n, nb, c.nbatch);
        } else if (c.K % 32 == 0 && aligned16 && !o.no_glds) {
            // (a 128 x 96 tile -- 10.3 instead of 6.2 rounds on the 1-hour stage-3 shape -- was measured at +2 %, inside run-to-run
            //  noise: the 160-wide tile stays.  That shape: 3168 tiles = 6.19 rounds of 2 workgroups per CU.)
            const int64_t slots = 2 * (int64_t)c.cus;
            const int64_t rem = nb % slots, full = nb - rem;
            int split = 0;
            // (a launch with less than a quarter of a round of tiles -- a few hundred rows -- is cut along K as a whole: its few
            //  tiles become up to 8x as many K slices, so that most of the chip takes part)
            // round: 4.45 us per K step + ~14 us per tile, scripts/bench_gemm_fit.py; fp16x3 form: 1.56 + ~10.5, scripts/ubench/gemm_f16x3.hip
            if (rem > 0 && (full > 0 || 4 * rem <= slots) && c.nbatch == 1 && c.mode <= 3 && c.has_ws && !o.no_splitk_tail)
                split = splitk_tail(rem, slots, nk, (size_t)128 * 160 * 4, c.splitk_ws_bytes, c.f16x3 ? 1.56 * nk + 10.5 : 4.45 * nk + 14.0);
            // One partial round of 160-wide tiles that already puts two workgroups on some CUs (256 < tiles <= 512) runs as long as
            // a full one.  When N is a multiple of 96 and the 5/3 as many 96-wide tiles still fit the round, they finish in ~0.6 of
            // it with every CU busy (5-minute clip, stage 3: 270 -> 450 tiles).  Same MFMA chain per output: bit-identical results.
            // (Only the layers that take the split epilogue: the generic one's row / column arithmetic is written for 160- and
            //  32-column waves.)
            const int64_t nb96 = cdiv(c.M, 128) * (c.N / 96);
            if (split < 2 && split_epilogue_ok(c, 96, (unsigned)c.nbatch) && !o.no_n96 && nb96 < (1ll << 31) &&
                glds_rounds_us(nb96, 0.6, slots, nk) < 0.95 * glds_rounds_us(nb, 1.0, slots, nk)) {
                plan_tiles(st, GK_GLDS, 128, 96, c.N / 96, nb96, 1);
            } else {
                plan_tiles(st, GK_GLDS, 128, 160, tiles_n, nb, c.nbatch);
                if (split >= 2) plan_tail(st, full, rem, split);
            }
            st.nsub = st.bn / 32;
            // the buffer form of the operand loads (default) needs the tile's lane offsets to fit 32 bits
            st.stage = c.f16x3 || (!o.global_loads && c.lda < (1 << 21) && c.ldw < (1 << 21)) ? 2 : 0;
            st.epi = split_epilogue_ok(c, st.bn, st.grid_y);
        } else {
            plan_tiles(st, GK_TILE_LARGE, bm, bn, tiles_n, nb, c.nbatch);
        }
        return p;
    }
}

}  // namespace tal
