// csrc/gconv_plan.h on the host: the grouped convs' launch plan over a sweep of entries, widths, group counts, lengths, batch sizes,
// forms, alignments, options and CU counts.  Per plan it checks what the kernels rely on (tiles cover T_out, whole group blocks, the
// two grid forms, LDS bytes by the kernels' own formulas, the split forms' channel conditions, the short-tile rule), per layout what
// the slab reads and the weight packer rely on, and prints, for tests/test_gconv_plan_cpu.py to hold against the parent's, behind a "C" line that
// names the case: one "L" line per launch or refusal, and for the first resize conv a "P" line with the answers of the 1 -> 10
// predicate.  At the end: "A <arm> <count>" per arm of the dispatcher.  Exits non-zero at the first violation.
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "../tal_asrd_amd/csrc/gconv_plan.h"

using namespace tal;

// ---- the sweep -------------------------------------------------------------------------------------------------------------------
static GconvCall call(int entry, int cus, int B, int64_t T, int C_in, int C_out, int groups, int ks = KS) {
    GconvCall c = {};
    c.entry = entry; c.cus = cus; c.B = B; c.T_in = T; c.C_in = C_in; c.C_out = C_out; c.groups = groups; c.ks = ks;
    c.has_y = entry != GE_C1_RES;
    c.has_y_split = c.x_split = entry == GE_C1_RES;
    c.o.short_below = 4;
    return c;
}

// every entry that takes a conv of `cig` -> `cog` channels per group (cig == cog: the TDSBlock conv, else the resize conv), in its
// plain form; T counts input rows (stride 2: both T and T + 1, so both parities)
template <class F>
static void entries(F&& f, int cus, int B, int64_t T, int cig, int cog, int groups) {
    const int ci = cig * groups, co = cog * groups;
    if (cig == cog) {
        for (int e : {GE_RES, GE_RES_F16X3, GE_RES_K}) f(call(e, cus, B, T, ci, co, groups));
        if (cig == 18) {      // the last stage's product form: split form in and out
            GconvCall c = call(GE_RES_F16X3, cus, B, T, ci, co, groups);
            c.x_split = c.has_y_split = true; c.has_y = false;
            f(c);
        }
    } else {
        for (int64_t t : {T, T + 1}) {
            for (int e : {GE_S2, GE_S2_F16X3, GE_S2_K}) f(call(e, cus, B, t, ci, co, groups));
            if (cig == 1) f(call(GE_C1_RES, cus, B, t, ci, co, groups));
        }
    }
}

static const int WIDTHS[][2] = {{1, 10}, {10, 14}, {14, 18}, {10, 10}, {14, 14}, {18, 18}};

template <class F>
static void sweep(F&& f) {
    // every length of the device guard test (T = 1..300 rows in; the resize convs: T and T + 1, so both parities)
    for (const auto& w : WIDTHS)
        for (int64_t T = 1; T <= 300; T += (w[0] == w[1] ? 1 : 2)) entries(f, 256, 1, T, w[0], w[1], 80);
    const int cu_counts[] = {64, 256, 304};
    for (int cus : cu_counts) {
        // the stock widths from one row to one hour (mel frames of a 30-second, 5-minute and 1-hour input and their stage lengths)
        const int64_t Ts[] = {1, 21, 64, 256, 257, 1491, 3001, 30001, 179991, 360001};
        for (const auto& w : WIDTHS)
            for (int B : {1, 2, 8, 64})
                for (int64_t T : Ts)
                    if (B == 1 || B == 8 || T == 3001 || T == 30001) entries(f, cus, B, T, w[0], w[1], 80);
        // other group counts; per-group widths without a specialised kernel
        for (int groups : {3, 8, 12, 16, 20, 40, 64, 80})
        {
            for (const auto& w : WIDTHS) entries(f, cus, 2, 3001, w[0], w[1], groups);
            entries(f, cus, 2, 3001, 4, 4, groups);
            entries(f, cus, 2, 3001, 2, 3, groups);
        }
        // every option, one at a time, where it is read: the matrix-core entries and the first resize conv
        for (int k = 0; k < 9; ++k)
            for (int B : {1, 8})
                for (int64_t T : {(int64_t)257, (int64_t)30001, (int64_t)360001})
                    for (const auto& w : WIDTHS)
                        entries([&](GconvCall c) {
                            if (c.entry == GE_RES || c.entry == GE_RES_K || c.entry == GE_S2_K || (c.entry == GE_S2 && c.C_in != c.groups)) return;
                            int* const field[] = {&c.o.c1_generic, &c.o.short_below, &c.o.short_below, &c.o.short_below, &c.o.no_shift18, &c.o.grid_xyz,
                                                  &c.o.long_tt,    &c.o.long_tt,     &c.o.long_tt};
                            const int value[] = {1, 0, 4, 1048576, 1, 1, 0, 128, 256};
                            *field[k] = value[k];
                            f(c);
                        }, cus, B, T, w[0], w[1], 80);
        // x off 16 bytes
        for (unsigned lo : {4u, 8u})
            for (const auto& w : WIDTHS)
                entries([&](GconvCall c) { c.x_lo = lo; f(c); }, cus, 1, 3001, w[0], w[1], 80);
        // every combination of split input, fp32 output and split output the matrix-core entries accept; 36 groups: C % 32 != 0
        for (int groups : {80, 36})
            for (int B : {1, 8})
                for (int64_t T : {(int64_t)64, (int64_t)360001})
                    for (const auto& w : WIDTHS)
                        for (int form = 0; form < 6; ++form) {
                            if (w[0] == 1) continue;
                            GconvCall c = call(w[0] == w[1] ? GE_RES_F16X3 : GE_S2_F16X3, cus, B, T, w[0] * groups, w[1] * groups, groups);
                            c.x_split = form >= 3;
                            c.has_y = form % 3 != 2;
                            c.has_y_split = form % 3 != 0;
                            f(c);
                        }
        // the first resize conv: split output and the folded mean, alone and together, where there is a kernel for them and where not
        for (int groups : {80, 40, 16, 8})
            for (int cog : {10, 14})
                for (int form = 1; form < 8; ++form)
                    for (int64_t T : {(int64_t)300, (int64_t)30001}) {
                        GconvCall c = call(GE_S2, cus, 2, T, (cog == 10 ? 1 : 10) * groups, cog * groups, groups);
                        c.has_y = !(form & 1); c.has_y_split = form & 1; c.has_in_mean = form & 2;
                        if (form & 4) c.o.c1_generic = 1;
                        f(c);
                    }
        // the any-k entries at other kernel sizes
        for (int ks : {1, 3, 8, 15, 21, 31, 63, 0, 64})
            for (int64_t T : {(int64_t)70, (int64_t)3001})
                for (const auto& w : WIDTHS) {
                    f(call(w[0] == w[1] ? GE_RES_K : GE_S2_K, cus, 2, T, w[0] * 80, w[1] * 80, 80, ks));
                    f(call(w[0] == w[1] ? GE_RES_K : GE_S2_K, cus, 2, T, w[0] * 6, w[1] * 6, 6, ks));
                }
        // bad shapes: no rows, no items, an input shorter than the kernel, channels that the groups do not divide
        for (const auto& w : WIDTHS)
            for (int v = 0; v < 3; ++v)
                entries([&](GconvCall c) {
                    if (v == 2 && c.entry == GE_C1_RES) return;       // (its channels are 1 and 10 per group by construction)
                    if (v == 2) c.C_in += 1, c.C_out += 1;
                    f(c);
                }, cus, v == 0 ? 0 : 1, v == 1 ? 0 : 3001, w[0], w[1], 80);
        // one batch item just under and just over the 2 GiB a buffer descriptor addresses
        for (const auto& w : WIDTHS) {
            const int C = w[0] == 1 ? w[1] * 80 : w[0] * 80;       // the channels of the rows the slab loads address
            const int64_t Tmax = (((int64_t)1 << 31) - 1 - (int64_t)300 * C * 4) / ((int64_t)C * 4);
            if (!gconv_f16x3_fits(Tmax, C) || gconv_f16x3_fits(Tmax + 1, C)) { printf("FAILED the 2 GiB bound is not where the sweep puts it\n"); exit(1); }
            for (int64_t T : {Tmax, Tmax + 1}) {
                if (w[0] == w[1]) f(call(GE_RES_F16X3, cus, 1, T, C, C, 80));
                else if (w[0] == 1) f(call(GE_C1_RES, cus, 1, 2 * (T - 1) + KS, 80, 800, 80));
                else f(call(GE_S2_F16X3, cus, 1, T, w[0] * 80, w[1] * 80, 80));
            }
        }
        // more than 2^31 workgroups: the plain 3-D grid
        f(call(GE_RES_F16X3, cus, 50000, 600000, 800, 800, 80));
        f(call(GE_RES_F16X3, cus, 45000, 600000, 800, 800, 80));
    }
}

// ---- checks ----------------------------------------------------------------------------------------------------------------------
#define CHECK(cond)                                                 \
    do {                                                            \
        if (!(cond)) {                                              \
            printf("FAILED %s (line %d)\n", #cond, __LINE__);       \
            exit(1);                                                \
        }                                                           \
    } while (0)

enum { A_VALU_1_10, A_VALU_10_14, A_VALU_14_18, A_VALU_RES_10, A_VALU_RES_14, A_VALU_RES_18, A_GENERIC_S2, A_GENERIC_RES, A_C1_LONG, A_C1_SHORT,
       A_C1_YSPLIT, A_C1_MEAN, A_MFMA_RES_10, A_MFMA_RES_14, A_MFMA_RES_18, A_MFMA_S2_10, A_MFMA_S2_14, A_MFMA_TT64, A_MFMA_TT128, A_MFMA_TT256,
       A_MFMA_RES_10_TT128, A_MFMA_RES_14_TT256, A_MFMA_SPLIT0, A_MFMA_SPLIT1, A_MFMA_SPLIT2, A_MFMA_XSPLIT, A_SHIFT18_LONG, A_SHIFT18_SHORT,
       A_SHIFT18_SWITCHED_OFF, A_C1RES_LONG, A_C1RES_SHORT, A_K_TILED_S2_10, A_K_TILED_S2_14, A_K_TILED_RES_10, A_K_TILED_RES_14, A_K_TILED_RES_18,
       A_K_C1_LONG, A_K_C1_SHORT, A_K_ANY_S2, A_K_ANY_RES, A_GRID_1D, A_GRID_3D_OPTION, A_GRID_3D_TOO_MANY, A_SHORT_TILES, A_LONG_TILES,
       A_R_NO_FOLD_KERNEL, A_R_NO_SPLIT_KERNEL, A_R_GROUPS, A_R_SHAPE, A_R_KSIZE, A_R_NO_MFMA_KERNEL, A_R_SPLIT_C, A_R_X_ALIGN, A_R_TOO_LARGE,
       A_R_SPLIT_OUT_C, A_R_SPLIT_IN_C, A_COUNT };
static const char* const arm_names[] = {
    "valu_1_10", "valu_10_14", "valu_14_18", "valu_res_10", "valu_res_14", "valu_res_18", "generic_s2", "generic_res", "c1_long", "c1_short",
    "c1_ysplit", "c1_mean", "mfma_res_10", "mfma_res_14", "mfma_res_18", "mfma_s2_10", "mfma_s2_14", "mfma_tt64", "mfma_tt128", "mfma_tt256",
    "mfma_res_10_tt128", "mfma_res_14_tt256", "mfma_split0", "mfma_split1", "mfma_split2", "mfma_xsplit", "shift18_long", "shift18_short",
    "shift18_switched_off", "c1res_long", "c1res_short", "k_tiled_s2_10", "k_tiled_s2_14", "k_tiled_res_10", "k_tiled_res_14", "k_tiled_res_18",
    "k_c1_long", "k_c1_short", "k_any_s2", "k_any_res", "grid_1d", "grid_3d_option", "grid_3d_too_many", "short_tiles", "long_tiles",
    "refused_no_fold_kernel", "refused_no_split_kernel", "refused_groups", "refused_shape", "refused_ksize", "refused_no_mfma_kernel",
    "refused_split_c", "refused_x_align", "refused_too_large", "refused_split_out_c", "refused_split_in_c"};
static long arms[A_COUNT];

// LDS bytes by the kernels' own declarations (csrc/gconv.hip, csrc/gconv_general.hip), written out independently of the plan's helpers
static size_t slab_halves(int pitch, int ntap, int nch, int rows) {
    const int nk = ((ntap - 1) * pitch + nch + 31) / 32, over = 32 * nk - ntap * pitch;
    return (size_t)((rows * pitch + (over > 0 ? over : 0) + 7) & ~7);
}
static size_t kernel_lds(const GconvLaunch& p, int ks) {
    const int tin = (p.tt - 1) * p.stride + ks;
    switch (p.kernel) {
        case GCK_VALU_TILED:
        case GCK_K_TILED: return (size_t)p.gb * p.cig * (tin | 1) * sizeof(float);                   // xs[CH][TINP]
        case GCK_K_C1: return ((size_t)tin * 20 + (size_t)ks * 200) * sizeof(float);                // xs[tin][NG] | wl[ks][NC]
        case GCK_MFMA: {                                                                            // slab[2 (hi, lo)][GB][GS]
            const int pitch = p.cig == 10 ? GC_P10 : p.cig == 18 ? GC_P18 : 16;
            const size_t gs = p.stride == 2 ? slab_halves(16, 11, p.cig, p.tt + 10) + slab_halves(16, 10, p.cig, p.tt + 9)
                                            : slab_halves(pitch, KS, p.cig, p.tt + KS - 1);
            return 2 * p.gb * gs * 2;
        }
        case GCK_C1_RES: return 2 * 4 * slab_halves(GC_P10, KS, 10, p.tt + KS - 1) * 2 + (size_t)(2 * (p.tt + KS - 2) + KS) * 4 * sizeof(float);
        case GCK_SHIFT18: return (2 * 2 * slab_halves(20, KS, 18, p.tt + KS - 1) + (size_t)2 * 4 * 768) * 2;   // | weight lines [GB][2][2][S18_WLP]
        default: return 0;
    }
}

static void print_case(const GconvCall& c) {
    printf("C entry=%d cus=%d B=%d T=%lld C=%d,%d groups=%d ks=%d x_lo=%u x_split=%d y=%d y_split=%d mean=%d opts=%d,%d,%d,%d,%d\n", c.entry, c.cus, c.B,
           (long long)c.T_in, c.C_in, c.C_out, c.groups, c.ks, c.x_lo, c.x_split, c.has_y, c.has_y_split, c.has_in_mean, c.o.c1_generic, c.o.short_below,
           c.o.no_shift18, c.o.grid_xyz, c.o.long_tt);
}

static void print_launch(const GconvLaunch& p, const GconvCall& c) {
    char name[96];
    const long long total = (long long)c.B * p.T_out * c.C_out;
    switch (p.kernel) {
        case GCK_VALU_TILED: snprintf(name, sizeof name, "valu<%d,%d,%d,%d,%d,%d>", p.cig, p.cog, p.stride, p.gb, p.tt, p.resid); break;
        case GCK_VALU_GENERIC: snprintf(name, sizeof name, "generic<%d>(%d,%d,%d,%lld)", p.resid, p.cig, p.cog, p.stride, total); break;
        case GCK_C1: snprintf(name, sizeof name, "c1<%d,%d,%d,%d>", p.cog, p.gb, p.tt, p.ysplit); break;
        case GCK_MFMA: snprintf(name, sizeof name, "mfma<%d,%d,%d,%d,%d,%d,%d,%d,0>", p.cig, p.cog, p.stride, p.resid, p.gb, p.tt, p.split, p.xsplit); break;
        case GCK_SHIFT18: snprintf(name, sizeof name, "shift18<%d>", p.tt); break;
        case GCK_C1_RES: snprintf(name, sizeof name, "mfma<%d,%d,%d,%d,%d,%d,%d,%d,1>", p.cig, p.cog, p.stride, p.resid, p.gb, p.tt, p.split, p.xsplit); break;
        case GCK_K_TILED: snprintf(name, sizeof name, "k<%d,%d,%d,%d,%d,%d>(%d)", p.cig, p.cog, p.stride, p.gb, p.tt, p.resid, c.ks); break;
        case GCK_K_C1: snprintf(name, sizeof name, "k_c1<%d,%d,%d>(%d)", p.cog, p.gb, p.tt, c.ks); break;
        default: snprintf(name, sizeof name, "k_any<%d>(%d,%d,%d,%d,%lld)", p.resid, p.cig, p.cog, p.stride, c.ks, total); break;
    }
    printf("L %s %u,%u,%u %u %zu %d,%d,%d %lld\n", name, p.grid_x, p.grid_y, p.grid_z, p.block, p.lds, p.n_tt, p.n_gb, p.nb_total, (long long)p.T_out);
}

static void check_and_print(const GconvCall& c) {
    print_case(c);
    if (c.entry == GE_S2)
        printf("P split=%d fold=%d\n", gconv_c1_ok(c.C_in, c.C_out, c.groups, c.x_lo, c.o.c1_generic != 0, true, false),
               gconv_c1_ok(c.C_in, c.C_out, c.groups, c.x_lo, c.o.c1_generic != 0, false, true));
    const GconvLaunch p = gconv_plan(c);
    if (p.refusal) {
        char text[160];
        gconv_refusal_text(c, p.refusal, text, sizeof text);
        printf("L refused: %s\n", text);
        CHECK(p.refusal >= GR_NO_FOLD_KERNEL && p.refusal <= GR_SPLIT_IN_C);
        ++arms[A_R_NO_FOLD_KERNEL + p.refusal - GR_NO_FOLD_KERNEL];
        return;
    }
    if (p.grid_x == 0) {        // no output element
        CHECK((int64_t)c.B * p.T_out * c.C_out == 0);
        printf("L none\n");
        return;
    }
    const bool mfma_family = p.kernel == GCK_MFMA || p.kernel == GCK_SHIFT18 || p.kernel == GCK_C1_RES;
    const bool per_element = p.kernel == GCK_VALU_GENERIC || p.kernel == GCK_K_ANY;
    const int ks = c.entry == GE_S2_K || c.entry == GE_RES_K ? c.ks : KS;
    const int64_t T_conv = c.entry == GE_C1_RES ? (c.T_in - KS) / 2 + 1 : c.T_in;      // rows the planned conv reads
    CHECK(p.T_out == (p.stride == 2 ? (T_conv - ks) / 2 + 1 : T_conv) && p.T_out > 0 && p.block == 256);
    CHECK(p.cig == (c.entry == GE_C1_RES ? 10 : c.C_in / c.groups) && p.cog == c.C_out / c.groups);
    CHECK(p.work == 2.0 * c.B * (double)p.T_out * c.C_out * (p.cig + (p.kernel == GCK_C1_RES)) * ks);
    CHECK(p.prof == (p.kernel == GCK_VALU_GENERIC ? GCP_NONE : p.resid ? GCP_RES : GCP_S2));
    if (per_element) {
        CHECK((int64_t)p.grid_x == cdiv((int64_t)c.B * p.T_out * c.C_out, 256) && p.grid_y == 1 && p.grid_z == 1 && p.lds == 0);
    } else {
        const int64_t tiles = cdiv(p.T_out, p.tt), group_blocks = c.groups / p.gb;
        CHECK(tiles * p.tt >= p.T_out && (tiles - 1) * p.tt < p.T_out);
        CHECK(group_blocks * p.gb == c.groups);
        if (p.n_tt > 0) {      // 1-D, XCD-ordered
            CHECK(mfma_family && p.n_gb > 0 && p.n_tt == tiles && p.n_gb == group_blocks && tiles * group_blocks * c.B < (1ll << 31));
            CHECK((int64_t)p.grid_x == tiles * group_blocks * c.B && p.grid_y == 1 && p.grid_z == 1);
            ++arms[A_GRID_1D];
        } else {
            CHECK(p.n_gb == 0 && (int64_t)p.grid_x == tiles && (int64_t)p.grid_y == group_blocks && (int64_t)p.grid_z == c.B);
            if (mfma_family) {
                CHECK(c.o.grid_xyz || tiles * group_blocks * c.B >= (1ll << 31));
                ++arms[c.o.grid_xyz ? A_GRID_3D_OPTION : A_GRID_3D_TOO_MANY];
            }
        }
        CHECK(p.lds == kernel_lds(p, ks) && p.lds <= 160 * 1024 && p.lds_reserve <= 160 * 1024);
        CHECK(p.lds_reserve == (p.kernel == GCK_K_TILED || p.kernel == GCK_K_C1 ? kernel_lds(p, TAL_GCONV_MAX_K) : p.lds));
    }
    CHECK(p.nb_total == (p.kernel == GCK_SHIFT18 && p.n_tt > 0 ? (int)p.grid_x : 0));
    if (mfma_family) {
        CHECK(gconv_f16x3_fits(T_conv, p.cig * c.groups) && gconv_has_mfma(p.cig * c.groups, p.cog * c.groups, c.groups, p.stride));
        CHECK(p.xsplit == c.x_split && p.split == (c.has_y ? (c.has_y_split ? 1 : 0) : 2));
        if (p.xsplit) CHECK((p.cig * c.groups) % 32 == 0 && (p.cig * p.gb) % 4 == 0);
        if (p.split) CHECK(c.C_out % 32 == 0);
        // short tiles exactly when the long ones give fewer than short_below x cus workgroups
        const int tt_long = p.stride == 2 ? 128 : 256;
        const bool few = cdiv(p.T_out, tt_long) * (c.groups / p.gb) * c.B < (int64_t)c.o.short_below * c.cus;
        CHECK((p.tt == 64) == few);
        ++arms[few ? A_SHORT_TILES : A_LONG_TILES];
    } else {
        CHECK(p.split == 0 && !p.xsplit && p.n_tt == 0);
    }
    if (p.ysplit) CHECK(p.kernel == GCK_C1 && c.C_out % 32 == 0);
    switch (p.kernel) {
        case GCK_VALU_TILED:
            CHECK(p.tt == (p.resid ? 256 : 128));
            ++arms[p.resid ? (p.cig == 10 ? A_VALU_RES_10 : p.cig == 14 ? A_VALU_RES_14 : A_VALU_RES_18)
                           : (p.cig == 1 ? A_VALU_1_10 : p.cig == 10 ? A_VALU_10_14 : A_VALU_14_18)];
            break;
        case GCK_VALU_GENERIC: ++arms[p.resid ? A_GENERIC_RES : A_GENERIC_S2]; break;
        case GCK_C1:
            CHECK(p.gb == 20 && (p.tt == 32) == (cdiv(p.T_out, 256) * (c.groups / 20) * c.B < 256) && (p.tt == 32 || p.tt == 256) && p.ysplit == c.has_y_split);
            ++arms[p.tt == 32 ? A_C1_SHORT : A_C1_LONG];
            if (p.ysplit) ++arms[A_C1_YSPLIT];
            if (c.has_in_mean) ++arms[A_C1_MEAN];
            break;
        case GCK_MFMA:
            CHECK(p.gb == (p.cig == 10 || (p.cig == 14 && p.stride == 1) ? 4 : 2) && p.resid == (p.stride == 1));
            ++arms[p.stride == 2 ? (p.cig == 10 ? A_MFMA_S2_10 : A_MFMA_S2_14) : p.cig == 10 ? A_MFMA_RES_10 : p.cig == 14 ? A_MFMA_RES_14 : A_MFMA_RES_18];
            ++arms[p.tt == 64 ? A_MFMA_TT64 : p.tt == 128 ? A_MFMA_TT128 : A_MFMA_TT256];
            if (p.stride == 1 && p.tt != 64) {
                CHECK(p.tt == (p.cig == 18 ? 256 : p.cig == 14 ? (c.o.long_tt == 256 ? 256 : 128) : (c.o.long_tt == 128 ? 128 : 256)));
                if (p.cig == 10 && p.tt == 128) ++arms[A_MFMA_RES_10_TT128];
                if (p.cig == 14 && p.tt == 256) ++arms[A_MFMA_RES_14_TT256];
            }
            ++arms[A_MFMA_SPLIT0 + p.split];
            if (p.xsplit) ++arms[A_MFMA_XSPLIT];
            if (p.cig == 18 && p.xsplit && p.split == 2) { CHECK(c.o.no_shift18); ++arms[A_SHIFT18_SWITCHED_OFF]; }
            break;
        case GCK_SHIFT18:
            CHECK(p.cig == 18 && p.gb == 2 && p.xsplit && p.split == 2 && !c.o.no_shift18 && (p.tt == 64 || p.tt == 256));
            ++arms[p.tt == 64 ? A_SHIFT18_SHORT : A_SHIFT18_LONG];
            break;
        case GCK_C1_RES:
            CHECK(p.gb == 4 && p.xsplit && p.split == 2 && (p.tt == 64 || p.tt == 256));
            ++arms[p.tt == 64 ? A_C1RES_SHORT : A_C1RES_LONG];
            break;
        case GCK_K_TILED:
            CHECK(p.tt == (p.resid ? 256 : 128) && (c.x_lo & 15) == 0);
            ++arms[p.resid ? (p.cig == 10 ? A_K_TILED_RES_10 : p.cig == 14 ? A_K_TILED_RES_14 : A_K_TILED_RES_18) : (p.cig == 10 ? A_K_TILED_S2_10 : A_K_TILED_S2_14)];
            break;
        case GCK_K_C1:
            CHECK(p.gb == 20 && (p.tt == 32) == (cdiv(p.T_out, 128) * (c.groups / 20) * c.B < 256) && (p.tt == 32 || p.tt == 128));
            ++arms[p.tt == 32 ? A_K_C1_SHORT : A_K_C1_LONG];
            break;
        default: ++arms[p.resid ? A_K_ANY_RES : A_K_ANY_S2]; break;
    }
    print_launch(p, c);
}

// what the slab reads and the weight packer rely on, for every layout with a kernel
static void check_layouts() {
    const int combos[][3] = {{10, 10, 1}, {14, 14, 1}, {18, 18, 1}, {10, 14, 2}, {14, 18, 2}, {1, 10, 2}, {4, 4, 1}, {18, 18, 2}, {10, 10, 2}};
    for (const auto& w : combos)
        for (int groups : {3, 4, 36, 80}) {
            const bool has = gconv_has_mfma(w[0] * groups, w[1] * groups, groups, w[2]);
            CHECK(has == (groups % 4 == 0 && w[0] >= 10 && w[1] == w[0] + (w[2] == 2 ? 4 : 0) && w[1] <= 18));
            CHECK((gconv_weight_table_bytes(w[0] * groups, w[1] * groups, groups, w[2]) > 0) == has);
            if (!has) continue;
            const GcLayout d = gc_layout(w[0], w[2], w[1], groups);
            CHECK(d.nseg == (w[2] == 2 ? 2 : 1) && d.mt_n == (w[1] + 15) / 16 && d.tapstep == w[2]);
            int taps = 0;
            for (int s = 0; s < d.nseg; ++s) {
                CHECK(32 * d.nk[s] >= (d.ntap[s] - 1) * d.pitch[s] + d.nch[s] && d.pitch[s] >= d.nch[s]);
                taps += d.ntap[s];
            }
            CHECK(taps == KS && (d.nseg == 2 || d.nk[1] == 0));
            CHECK(d.perm_nk % 4 == 0 && d.perm_nk <= d.nk[0] && (d.perm_nk > 0) == d.perm());
            // the packer writes one hi and one lo half per element of [g][mt][K chunk][lane][8]
            const size_t elements = (size_t)groups * d.mt_n * (d.nk[0] + d.nk[1]) * 64 * 8;
            const bool shift18 = w[0] == 18 && w[1] == 18 && w[2] == 1;
            CHECK(d.has_shift18() == shift18);
            CHECK(gconv_weight_table_bytes(w[0] * groups, w[1] * groups, groups, w[2]) == 2 * elements * 2 + (shift18 ? (size_t)groups * 2 * 2 * 768 * 2 : 0));
        }
    CHECK(S18_WLP == 768 && S18_WL <= S18_WLP && S18_WPRE == 140);
}

int main() {
    static_assert(sizeof(arm_names) / sizeof(arm_names[0]) == A_COUNT, "one name per arm");
    check_layouts();
    long cases = 0;
    sweep([&](const GconvCall& c) {
        check_and_print(c);
        ++cases;
    });
    for (int a = 0; a < A_COUNT; ++a) printf("A %s %ld\n", arm_names[a], arms[a]);
    printf("cases %ld\n", cases);
    return 0;
}
