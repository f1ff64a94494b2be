// csrc/gemm_plan.h on the host: the dense layers' launch plan over a sweep of shapes, flags, alignments, options and CU counts.
// Per plan it checks what the kernels rely on (rows tiled in order, grid = whole tiles + K slices, slices inside the scratch, exact
// magic divisors, step bound) and prints one "L" line per launch, in the format of tests/gemm_plan_parent.txt, behind a "C" line
// that names the case.  At the end: "A <arm> <count>" per arm of the dispatcher.  Exits non-zero at the first violation.
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>
#include <string>

#include "../tal_asrd_amd/csrc/gemm_plan.h"

using namespace tal;

// ---- the sweep -------------------------------------------------------------------------------------------------------------------
static const size_t WS = (size_t)1024 * 128 * 160 * 4;      // gemm_splitk_ws_bytes()

// a TDS layer as launch_linear_f16x3 passes it: packed rows, 16-byte pointers, scratch; modes 1 / 2 in the split form under the guard
static GemmCall layer(int cus, int64_t M, int N, int K, int mode, bool f16x3 = true) {
    GemmCall c = {};
    c.M = M; c.N = N; c.K = K; c.mode = mode; c.nbatch = 1;
    c.f16x3 = f16x3;
    c.out_split = f16x3 && (mode == 1 || mode == 2) && N % 160 == 0;
    c.res_split = c.out_split && mode == 2;
    c.has_range_flag = c.out_split;
    c.lda = K; c.ldw = K; c.ldy = N; c.ldres = N;
    c.has_ws = true;
    c.splitk_ws_bytes = WS;
    c.cus = cus;
    c.o.s64_below = 2;
    return c;
}

template <class F>
static void sweep(F&& f) {
    const int cu_counts[] = {64, 256, 304};
    for (int cus : cu_counts) {
        const int64_t round = 256 * (int64_t)cus;
        // the TDS widths over short to one-hour inputs, relu and residual layers (64 x 80 in both heights and orders, row split with
        // both landings, 128 x 160 whole / sliced / all-sliced, 128 x 96, 256 x 160 whole and sliced)
        const int64_t Ms[] = {129, 200, 376, 700, 751, 1000, 1819, 3000, 3300, 5000, 8000, 13057, 45000, round + 3, round + 5000, round + 9000, 3 * round + 700};
        const int widths[] = {800, 1120, 1440};
        for (int C : widths)
            for (int mode = 1; mode <= 2; ++mode)
                for (int64_t M : Ms) f(layer(cus, M, C, C, mode));
        // every option, one at a time, on the widest layer
        for (int k = 0; k < 12; ++k)
            for (int64_t M : {(int64_t)376, (int64_t)1819, (int64_t)5000, round + 3, round + 5000, 3 * round + 700}) {
                GemmCall c = layer(cus, M, 1440, 1440, 1 + k % 2);
                int* const field[] = {&c.o.s64_below, &c.o.no_w64, &c.o.no_glds, &c.o.no_splitk_tail, &c.o.no_row_split, &c.o.no_n96, &c.o.global_loads,
                                      &c.o.s64_rows, &c.o.s64_rows, &c.o.s64_order, &c.o.s64_order, &c.o.w64_stagger};
                const int value[] = {0, 1, 1, 1, 1, 1, 1, 1, 2, 1, 2, 50};
                *field[k] = value[k];
                f(c);
            }
        // the split epilogue refused at each of its sites: fp32 output, no range flag, fp32 residual, Y off 16 bytes, a row pitch
        // that is no multiple of 4 (there the row split's remainder is derived from the pitch), modes 0 and 3, no scratch
        for (int v = 0; v < 9; ++v)
            for (int64_t M : {(int64_t)700, (int64_t)1819, (int64_t)5000, (int64_t)8000, round + 3, round + 2000, round + 5000}) {
                GemmCall c = layer(cus, M, 1440, v == 7 ? 96 : 1440, v == 2 ? 2 : v == 5 ? 0 : v == 6 ? 3 : 1);
                if (v == 0 || v == 3 || v == 4) c.out_split = c.has_range_flag = false;
                if (v == 1) c.has_range_flag = false;
                if (v == 2) c.res_split = false;
                if (v == 3) c.y_lo = 8;
                if (v == 4) c.ldy = 1442, c.ldres = 1446;
                if (v == 6) c.has_ws = false, c.splitk_ws_bytes = 0;
                if (v == 8) c.bias_lo = 4;
                f(c);
            }
        // the shapes the GPU tests name
        for (int K = 32; K <= 256; K += 32) f(layer(cus, round + 3, 160, K, 1));
        f(layer(cus, round + 5000, 160, 256, 1));
        for (int K : {96, 256, 800}) f(layer(cus, 8000, 800, K, 1));
        for (int N : {800, 1440}) {
            GemmCall c = layer(cus, 700, N, 256, 1);
            c.o.s64_below = 0;
            f(c);
        }
        f(layer(cus, 1819, 1440, 96, 1));
        f(layer(cus, 376, 1440, 1440, 2));
        f(layer(cus, 751, 1120, 1120, 2));
        // a scratch buffer too small for the tail search's first, or later, candidates
        for (size_t bytes : {(size_t)0, (size_t)16, WS / 64, WS / 8}) {
            GemmCall c = layer(cus, round + 5000, 1440, 1440, 1);
            c.splitk_ws_bytes = bytes;
            f(c);
            c = layer(cus, 3300, 800, 800, 1);
            c.splitk_ws_bytes = bytes;
            f(c);
        }
        // exact fp32 layers: the one-hour stage-3 shape (3168 tiles of 128 x 160), the heads, the decoder's short problems, batches
        for (int mode = 0; mode <= 4; ++mode)
            for (int64_t M : {(int64_t)1, (int64_t)100, (int64_t)512, (int64_t)513, (int64_t)3000, (int64_t)45000})
                for (int nbatch : {1, 8}) {
                    GemmCall c = layer(cus, M, mode == 4 ? 6008 : 1440, mode == 4 ? 128 : 1440, mode, false);
                    c.nbatch = nbatch;
                    f(c);
                }
        // the register tiles: K < 256 and K >= 256 below 513 rows (mode 4, a misaligned operand, gemm_no_splitk4), the large one
        // through K % 32 != 0, a misaligned operand and gemm_no_glds; the global form of the operand loads through a long pitch
        for (int v = 0; v < 5; ++v)
            for (int64_t M : {(int64_t)40, (int64_t)512, (int64_t)700, (int64_t)5000})
                for (int K : {36, 128, 256, 2048}) {
                    GemmCall c = layer(cus, M, 800, K, v == 4 ? 2 : 0, false);
                    if (v == 1) c.a_lo = 4;
                    if (v == 2) c.w_lo = 8;
                    if (v == 3) c.o.no_splitk4 = c.o.no_glds = 1;
                    if (v == 4) c.lda = (int64_t)1 << 21;
                    f(c);
                }
        // too many 128-row tiles for the 32-bit tile arithmetic: refused; as 256-row tiles of the fp16x3 form they still fit
        f(layer(cus, (int64_t)1 << 22, 64000, 32, 0, false));
        f(layer(cus, (int64_t)1 << 22, 64000, 32, 0));
    }
}

// ---- one line per launch ---------------------------------------------------------------------------------------------------------
static std::string kernel_name(const GemmStep& st, const GemmCall& c) {
    char b[64];
    const int mode = c.mode;
    const int m3 = mode < 3 ? mode : 3;
    switch (st.kernel) {
        case GK_S64: snprintf(b, sizeof b, "s64<%d,%d>", mode, st.waves); break;
        case GK_W64: snprintf(b, sizeof b, "w64<%d,%d,%d>", m3, (int)st.splitk, st.epi); break;
        case GK_GLDS: snprintf(b, sizeof b, "glds<%d,%d,%d,%d,%d,%d>", st.splitk ? m3 : mode, st.nsub, (int)st.splitk, st.stage, (int)c.f16x3, st.epi); break;
        case GK_SPLITK4: snprintf(b, sizeof b, "splitk4<%d,4>", m3); break;
        case GK_TILE_K256: snprintf(b, sizeof b, "tile<%d,1,1,128>", mode); break;
        case GK_TILE_SMALL: snprintf(b, sizeof b, "tile<%d,1,1,32>", mode); break;
        default: snprintf(b, sizeof b, "tile<%d,4,5,32>", mode); break;
    }
    return b;
}

static void print_launch(const std::string& name, unsigned gx, unsigned gy, unsigned block, const GemmStep& st, int ticks, int blocks) {
    printf("L %s %u,%u %u %lld %lld %d %d %d %d %d %d %d,%d\n", name.c_str(), gx, gy, block, (long long)st.rows, (long long)st.row0, st.tiles_n,
           st.tiles_m, st.n_major, st.tile_base, st.split, st.tail_tiles, ticks, blocks);
}

static long arms[64];
static const char* const arm_names[] = {
    "s64_2waves", "s64_4waves", "s64_m_major", "s64_n_major", "w64_whole", "w64_ktail", "row_split_to_s64", "row_split_to_128", "glds160_whole",
    "glds160_ktail_behind_rounds", "glds_all_sliced", "glds96", "epi_glds_taken", "epi_glds_refused", "epi_w64_taken", "epi_w64_refused",
    "epi_n96_taken", "epi_n96_refused", "loads_buffer", "loads_global", "splitk4", "tile_k256", "tile_small", "tile_large_ktail",
    "tile_large_misaligned", "tile_large_no_glds", "mode4_small", "mode4_large", "batched", "stagger", "refused"};
enum { A_S64_2, A_S64_4, A_S64_M, A_S64_N, A_W64, A_W64_TAIL, A_RS_S64, A_RS_128, A_G160, A_G160_TAIL, A_G_SLICED, A_G96, A_EG_T, A_EG_R, A_EW_T,
       A_EW_R, A_E96_T, A_E96_R, A_LD_BUF, A_LD_GLOBAL, A_SPLITK4, A_T256, A_TSMALL, A_TL_K, A_TL_MIS, A_TL_NOGLDS, A_M4_SMALL, A_M4_LARGE,
       A_BATCHED, A_STAGGER, A_REFUSED, A_COUNT };

static unsigned umulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }

static bool magic_holds(int64_t nb, int d, unsigned magic) {
    if (d == 1) return true;        // the kernels skip the multiply
    auto ok = [&](int64_t t) { return t < 0 || t >= nb || umulhi((unsigned)t, magic) == (unsigned)(t / d); };
    if (!(ok(0) && ok(d - 1) && ok(d) && ok(nb - 1))) return false;
    for (int64_t t = d; t <= nb; t += d)
        if (!(ok(t - 1) && ok(t) && ok(t + 1))) return false;
    return true;
}

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            printf("FAILED %s (step %d of the case above)\n", #cond, i); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

static void check_and_print(const GemmCall& c) {
    const GemmOpts& o = c.o;
    printf("C cus=%d M=%lld N=%d K=%d mode=%d nbatch=%d f16x3=%d out_split=%d res_split=%d ld=%lld,%lld,%lld,%lld ws=%d:%zu flag=%d lo=%u,%u,%u,%u,%u "
           "opts=%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d\n", c.cus, (long long)c.M, c.N, c.K, c.mode, c.nbatch, c.f16x3, c.out_split, c.res_split,
           (long long)c.lda, (long long)c.ldw, (long long)c.ldy, (long long)c.ldres, c.has_ws, c.splitk_ws_bytes, c.has_range_flag, c.a_lo, c.w_lo, c.y_lo,
           c.res_lo, c.bias_lo, o.s64_below, o.no_w64, o.no_glds, o.no_splitk4, o.no_splitk_tail, o.no_row_split, o.no_n96, o.global_loads, o.s64_rows,
           o.s64_order, o.w64_stagger);
    const GemmPlan p = gemm_plan(c);
    int i = 0;
    if (p.grid_too_large) {
        printf("L refused\n");
        ++arms[A_REFUSED];
        return;
    }
    CHECK(p.n >= 1 && p.n <= GEMM_PLAN_MAX_STEPS);
    int64_t next_row = 0;
    double work = 0.0;
    for (i = 0; i < p.n; ++i) {
        const GemmStep& st = p.step[i];
        CHECK(st.row0 == next_row && st.rows > 0);
        next_row += st.rows;
        work += st.work;
        const int64_t tiles = cdiv(st.rows, st.bm) * st.tiles_n;
        CHECK(st.tiles_n == cdiv(c.N, st.bn) && st.grid_y == (unsigned)c.nbatch);
        if (st.split == 0) {
            CHECK(!st.splitk && st.tile_base == 0 && st.tail_tiles == 0 && st.fixup_grid == 0 && (int64_t)st.grid_x == tiles);
        } else {
            CHECK(st.splitk && st.split >= 2 && st.split <= 8 && st.split <= (c.K / 32) / 4 && st.tail_tiles > 0);
            CHECK((int64_t)st.tile_base + (int64_t)st.tail_tiles * st.split == (int64_t)st.grid_x && (int64_t)st.tile_base + st.tail_tiles == tiles);
            CHECK((size_t)st.tail_tiles * st.split * st.bm * 160 * 4 <= c.splitk_ws_bytes && st.bn == 160 && c.has_ws);
            CHECK(st.fixup_grid == (unsigned)st.tail_tiles * (st.bm / 32));
        }
        CHECK(tiles < (1ll << 31) && (int64_t)st.grid_x < (1ll << 31));
        CHECK(st.tiles_n_magic == magic_of(st.tiles_n) && magic_holds(tiles, st.tiles_n, st.tiles_n_magic));
        if (st.kernel == GK_S64) CHECK(st.tiles_m == cdiv(st.rows, st.bm) && st.tiles_m_magic == magic_of(st.tiles_m) && magic_holds(tiles, st.tiles_m, st.tiles_m_magic));
        else CHECK(st.tiles_m == 0 && st.n_major == 0);

        const bool last = i == p.n - 1, tds = c.f16x3 && (c.mode == 1 || c.mode == 2);
        switch (st.kernel) {
            case GK_S64:
                ++arms[st.waves == 2 ? A_S64_2 : A_S64_4];
                ++arms[st.n_major ? A_S64_N : A_S64_M];
                if (i > 0) ++arms[A_RS_S64];
                CHECK(st.block == 64u * st.waves && st.bm == 16 * st.waves);
                break;
            case GK_W64:
                ++arms[st.split ? A_W64_TAIL : A_W64];
                if (tds) ++arms[st.epi ? A_EW_T : A_EW_R];
                if (st.stagger_ticks > 0) ++arms[A_STAGGER];
                CHECK(last || st.split == 0);
                break;
            case GK_GLDS:
                if (i > 0) ++arms[A_RS_128];
                ++arms[st.bn == 96 ? A_G96 : st.split == 0 ? A_G160 : st.tile_base > 0 ? A_G160_TAIL : A_G_SLICED];
                ++arms[st.stage == 2 ? A_LD_BUF : A_LD_GLOBAL];
                if (tds && st.bn == 160) ++arms[st.epi ? A_EG_T : A_EG_R];
                if (tds && st.split == 0 && c.N % 96 == 0 && !o.no_n96)
                    ++arms[split_epilogue_ok(c, 96, st.grid_y) ? A_E96_T : A_E96_R];
                if (c.mode == 4) ++arms[A_M4_LARGE];
                CHECK(st.nsub * 32 == st.bn && (st.bn == 160 || (st.epi == 1 && st.split == 0)));
                break;
            case GK_SPLITK4: ++arms[A_SPLITK4]; break;
            case GK_TILE_K256:
            case GK_TILE_SMALL:
                ++arms[st.kernel == GK_TILE_K256 ? A_T256 : A_TSMALL];
                if (c.mode == 4) ++arms[A_M4_SMALL];
                break;
            default:
                if (c.K % 32 != 0) ++arms[A_TL_K];
                else if (((c.a_lo | c.w_lo) & 15) != 0) ++arms[A_TL_MIS];
                else { CHECK(o.no_glds); ++arms[A_TL_NOGLDS]; }
                break;
        }
        if (st.kernel != GK_S64) CHECK(st.block == 256);
        if (st.kernel != GK_W64) CHECK(st.stagger_ticks == 0 && st.stagger_blocks == 0);
        if (c.nbatch > 1) ++arms[A_BATCHED];
        print_launch(kernel_name(st, c), st.grid_x, st.grid_y, st.block, st, st.stagger_ticks, st.stagger_blocks);
        if (st.fixup_grid) {
            char b[32];
            snprintf(b, sizeof b, "fixup<%d,5,%d>", c.mode, st.bm);
            print_launch(b, st.fixup_grid, 1, 256, st, 0, 0);
        }
    }
    i = p.n;
    CHECK(next_row == c.M);
    CHECK(work == 2.0 * (double)c.M * (double)c.N * (double)c.K * c.nbatch);
}

int main() {
    static_assert(sizeof(arm_names) / sizeof(arm_names[0]) == A_COUNT, "one name per arm");
    long cases = 0;
    sweep([&](const GemmCall& c) {
        check_and_print(c);
        ++cases;
    });
    for (int a = 0; a < A_COUNT; ++a) printf("A %s %ld\n", arm_names[a], arms[a]);
    printf("cases %ld\n", cases);
    return 0;
}
