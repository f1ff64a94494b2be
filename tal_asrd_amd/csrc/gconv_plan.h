// What a grouped-conv entry point (csrc/gconv.hip, csrc/gconv_general.hip) launches: the K-segment layout of the matrix-core
// kernels, the "is there a kernel" predicates, and per call the kernel family, template choices, grid, LDS bytes and profiling
// scope -- or the refusal -- decided from the call's shape, flags, address alignment, CU count and options alone.  Plain C++ (no
// HIP types, no pointer dereferenced, no heap; the plan comes back by value), so that tests/test_gconv_plan_cpu.py can walk every
// arm with a host compiler.  A launcher checks its pointers, fills a GconvCall, asks for the plan and hands it to one helper that
// maps it to the instantiation.  Every grouped-conv call is exactly one launch.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/tal_asrd.h"
#include "gemm_plan.h"      // cdiv

namespace tal {

constexpr int KS = 21;      // the reference's default kernel size: every kernel of gconv.hip is built for it

// slab row pitch (halves) of a 10-channel group: 10 = compact (20-byte rows: every fragment read is 4-byte aligned and half
// of the LDS cycles are bank conflicts), 12 = 24-byte rows (8-byte aligned reads, one more K chunk of 32)
#ifndef GC_P10
#define GC_P10 12
#endif
#ifndef GC_P18
#define GC_P18 20
#endif
// K permutation of the fragment reads (GcLayout::perm); 0: plain order (ablation)
#ifndef GC_KPERM
#define GC_KPERM 1
#endif

// K-segment layout of gconv_mfma_kernel for (C_in/G, stride): compile-time constants in the kernels (constexpr GcLayout LY =
// gc_layout(..)) and, with the call's C_out/G and group count, the run-time argument of the weight packer.
struct GcLayout {
    int nseg, pitch[2], ntap[2], nch[2], choff[2], tap0[2], nk[2], tapstep, cig, cog, mt_n, groups;
    int perm_nk;      // K chunks of segment 0 in the permuted order (perm())
    // K permutation against LDS bank conflicts (single-segment stride-1 layouts whose rows are an ODD number of 8-byte bank
    // pairs apart: 12 or 20 halves).  Lanes 0-31 of a fragment read are 16 output steps x 2 k groups; with the k groups 16
    // bytes apart every such read is a 2-way conflict (p * d = 4 mod 64 banks has a solution |d| <= 15 for p = 6, 10: SQ_LDS_
    // BANK_CONFLICT = 48 % of the LDS cycles, the LDS array 70-75 % busy); 128 bytes apart it is conflict-free -- the 16 rows
    // fill every other bank pair, the second k group the rest.  So inside a block of 128 slab halves (4 K chunks) MFMA j takes
    // its k groups 0..3 from the 16-byte pieces j, j + 8, j + 4, j + 12; the weights are packed with the same permutation
    // (pack_gconv_mfma_kernel).  Chunks behind the last whole block of four keep the plain order.
    constexpr bool perm() const { return nseg == 1 && tapstep == 1 && pitch[0] % 8 == 4 && GC_KPERM; }
    constexpr int nks() const { return nk[0] + nk[1]; }
    constexpr int rows(int s, int tt) const { return tapstep == 2 ? tt + ntap[s] - 1 : tt + KS - 1; }
    constexpr int slab(int s, int tt) const {        // halves, incl. the K round-up the last output step reads past its window
        if (s >= nseg) return 0;
        const int over = 32 * nk[s] - ntap[s] * pitch[s];
        return (rows(s, tt) * pitch[s] + (over > 0 ? over : 0) + 7) & ~7;
    }
    // halves of the [g][mt][K chunk][hi, lo][lane][8] fragment table; the 18-channel stride-1 conv keeps a second table behind it:
    // the weight lines of its two left-over channels (gconv18_shift_kernel, pack_gconv_shift18_kernel)
    constexpr size_t main_halves() const { return (size_t)groups * mt_n * nks() * 2 * 64 * 8; }
    constexpr bool has_shift18() const { return cig == 18 && cog == 18 && tapstep == 1 && nseg == 1 && pitch[0] == 20; }
};

constexpr GcLayout gc_layout(int cig, int stride, int cog = 0, int groups = 0) {
    // 18 channels per group, stride 1: one segment of 40-byte rows (GC_P18 = 20: 14 K chunks, 8-byte aligned fragment reads;
    // -10 % on the kernel alone, -0.5 % on the 1-hour step) or, with GC_P18 = 0, two K segments (16 channels at pitch 16 + 2 at
    // pitch 8: 17 K chunks, every fragment one aligned 16-byte read -- round 1's form; a 48-byte pitch lost 37 % to bank conflicts)
    const bool split18 = cig > 16 && stride == 1 && GC_P18 == 0;
    GcLayout d = {};
    d.nseg = (stride == 2 || split18) ? 2 : 1;
    for (int s = 0; s < 2; ++s) {
        d.pitch[s] = stride == 2 ? 16 : (split18 ? (s == 0 ? 16 : 8) : (cig > 16 ? GC_P18 : (cig == 10 ? GC_P10 : 16)));
        d.ntap[s] = stride == 2 ? (s == 0 ? (KS + 1) / 2 : KS / 2) : KS;
        d.nch[s] = split18 ? (s == 0 ? 16 : cig - 16) : cig;
        d.choff[s] = (split18 && s == 1) ? 16 : 0;
        d.tap0[s] = stride == 2 ? s : 0;
        d.nk[s] = s < d.nseg ? ((d.ntap[s] - 1) * d.pitch[s] + d.nch[s] + 31) / 32 : 0;
    }
    d.tapstep = stride; d.cig = cig; d.cog = cog; d.mt_n = (cog + 15) / 16; d.groups = groups;
    d.perm_nk = d.perm() ? (d.nk[0] / 4) * 4 : 0;
    return d;
}

// gconv18_shift_kernel's weight lines (the constants the host needs for LDS and weight-table sizes; the rest sits beside the kernel)
constexpr int S18_NKA = 18;      // K chunks of the shifted tile: (21 + 7) rows x 20 halves = 560 -> 576
constexpr int S18_SH = 8;        // shifts per channel
constexpr int S18_WPRE = 20 * (S18_SH - 1);                   // 140
constexpr int S18_WL = S18_WPRE + 32 * S18_NKA + 8;           // 724 halves per line, rounded up so that a workgroup's eight lines are
constexpr int S18_WLP = (S18_WL + 255) & ~255;                // a whole number of 256 x 16-byte pieces (768)

// ---- predicates, each written once ----------------------------------------------------------------------------------------------
// is there a matrix-core kernel (and a fragment table) for these channels: 10 / 14 / 18 per group at stride 1, 10 -> 14 and
// 14 -> 18 at stride 2, groups in fours
inline bool gconv_has_mfma(int C_in, int C_out, int groups, int stride) {
    if (groups <= 0 || C_in % groups || C_out % groups || groups % 4) return false;
    const int cig = C_in / groups, cog = C_out / groups;
    if (stride == 1) return cig == cog && (cig == 10 || cig == 14 || cig == 18);
    return stride == 2 && ((cig == 10 && cog == 14) || (cig == 14 && cog == 18));
}
// bytes of the fragment table (+ the shift-18 weight lines), 0 without a kernel
inline size_t gconv_weight_table_bytes(int C_in, int C_out, int groups, int stride) {
    if (!gconv_has_mfma(C_in, C_out, groups, stride)) return 0;
    const GcLayout d = gc_layout(C_in / groups, stride, C_out / groups, groups);
    return d.main_halves() * 2 + (d.has_shift18() ? (size_t)groups * 4 * S18_WLP * 2 : 0);
}
// does gconv_s2_c1_kernel (1 mel bin -> 10 channels per group, groups in twenties, 16-byte rows) take this call?  split_out: the
// output in the hi / lo split form, which is laid out in 32-channel blocks.  fold_mean: the input's mean folded into the bias --
// the conv has no padding, so it adds no condition of its own.
inline bool gconv_c1_ok(int C_in, int C_out, int groups, unsigned x_lo, bool c1_generic, bool split_out, bool fold_mean) {
    (void)fold_mean;
    return groups > 0 && C_in == groups && C_out == 10 * groups && groups % 20 == 0 && C_in % 4 == 0 && (!split_out || C_out % 32 == 0) &&
           (x_lo & 15) == 0 && !c1_generic;
}
// the first resize conv (1 -> 10 channels per group) computed inside the first TDSBlock conv's launch (gconv_mfma_kernel<.., FROMC1>)
inline bool gconv_c1_res_fusable(int C_in, int C_out, int groups, unsigned mel_lo) {
    return groups > 0 && C_in == groups && C_out == 10 * groups && groups % 4 == 0 && C_out % 32 == 0 && (mel_lo & 15) == 0 &&
           gconv_has_mfma(C_out, C_out, groups, 1);
}
// the slab loads address one batch item ([T, C] floats) through a buffer descriptor with 32-bit byte offsets
inline bool gconv_f16x3_fits(int64_t T, int C) { return T * C * 4 + (int64_t)300 * C * 4 < ((int64_t)1 << 31); }
// Short inputs: tiles of 64 output steps instead of 256 (128 for stride 2) when the long tiles would not give every CU
// gconv_short_below workgroups (option "gconv_short_below", default 4: two rounds of two resident workgroups) -- a wave then
// walks 4 blocks of 16 steps instead of 16 behind its slab fill, on 4x the workgroups.  Same arithmetic per output: results
// do not depend on the tile length.
inline bool gconv_short_tiles(int64_t T_out, int tt_long, int group_blocks, int B, int short_below, int cus) {
    return cdiv(T_out, tt_long) * group_blocks * B < (int64_t)short_below * cus;
}

// ---- the plan -------------------------------------------------------------------------------------------------------------------
// the grouped-conv switches of tal_set_option, read once per call
struct GconvOpts {
    int c1_generic, short_below, no_shift18, grid_xyz, long_tt;
};

enum GconvEntry { GE_S2, GE_RES, GE_S2_F16X3, GE_RES_F16X3, GE_C1_RES, GE_S2_K, GE_RES_K };

// The facts of a call the decisions rest on.  T_in: input rows (GE_C1_RES: of the log-mel, with C_in = groups mel bins and
// C_out = 10 groups); ks: the any-k entries' kernel size (KS elsewhere); x_lo: the low four address bits of x.  The launcher
// has checked the pointers: there is an output, and x is not an output.
struct GconvCall {
    int entry;                      // GconvEntry
    int B;
    int64_t T_in;
    int C_in, C_out, groups, ks;
    unsigned x_lo;
    bool x_split, has_y, has_y_split, has_in_mean;
    int cus;
    GconvOpts o;
};

enum GconvKernel {
    GCK_VALU_TILED,     // gconv_kernel<CIG, COG, STRIDE, GB, TT, RESID>
    GCK_VALU_GENERIC,   // gconv_generic_kernel<RESID>: one thread per output element
    GCK_C1,             // gconv_s2_c1_kernel<10, NG, TT, YSPLIT>
    GCK_MFMA,           // gconv_mfma_kernel<CIG, COG, STRIDE, RESID, GB, TT, SPLIT, XSPLIT>
    GCK_SHIFT18,        // gconv18_shift_kernel<TT>
    GCK_C1_RES,         // gconv_mfma_kernel<10, 10, 1, true, 4, TT, 2, true, FROMC1 = true>
    GCK_K_TILED,        // gconv_k_kernel<CIG, COG, STRIDE, GB, TT, RESID>
    GCK_K_C1,           // gconv_k_c1_kernel<10, NG, TT>
    GCK_K_ANY           // gconv_k_any_kernel<RESID>
};

// why a call is refused (the message texts: gconv_refusal_text below)
enum GconvRefusal {
    GR_NONE, GR_NO_FOLD_KERNEL, GR_NO_SPLIT_KERNEL, GR_GROUPS, GR_SHAPE, GR_KSIZE, GR_NO_MFMA_KERNEL, GR_SPLIT_C, GR_X_ALIGN, GR_TOO_LARGE,
    GR_SPLIT_OUT_C, GR_SPLIT_IN_C
};

constexpr int GCP_NONE = -1, GCP_RES = 1, GCP_S2 = 2;       // profiling scope: none, PROF_GCONV_RES, PROF_GCONV_S2

struct GconvLaunch {
    int refusal;                    // GconvRefusal; != GR_NONE: nothing is launched
    int kernel;                     // GconvKernel
    int cig, cog, stride, gb, tt;   // gb: groups per workgroup (GB, or NG of the 1 -> 10 kernels; 0: one thread per element)
    bool resid;
    int split;                      // matrix-core kernels: 0 = fp32 output, 1 = fp32 + its hi / lo split, 2 = the split form only
    bool xsplit, ysplit;            // ysplit: GCK_C1 writes the split form
    unsigned grid_x, grid_y, grid_z, block;     // grid_x == 0: no output element, nothing to launch
    int n_tt, n_gb, nb_total;       // > 0: the 1-D XCD-ordered grid (GC_BLOCK_INDEX); nb_total: GCK_SHIFT18's logical block count
    size_t lds, lds_reserve;        // dynamic LDS of this launch; what the instantiation reserves once (the any-k kernels: at k = 63)
    int prof;                       // GCP_*
    double work;                    // flops of the profiling scope
    int64_t T_out;
};

// LDS bytes, as the kernels lay them out
inline size_t gconv_valu_lds(int cig, int gb, int tt, int stride, int ks) { return (size_t)gb * cig * (size_t)(((tt - 1) * stride + ks) | 1) * 4; }
inline size_t gconv_k_c1_lds(int tt, int ks) { return ((size_t)((tt - 1) * 2 + ks) * 20 + (size_t)ks * 20 * 10) * 4; }
inline size_t gconv_mfma_lds(const GcLayout& ly, int gb, int tt) { return (size_t)2 * gb * (ly.slab(0, tt) + ly.slab(1, tt)) * 2; }
inline size_t gconv_c1_res_lds(int tt) {       // the slabs + the mel rows behind tt + 20 rows of the stage: [2 (tt + 19) + 21][4] floats
    return gconv_mfma_lds(gc_layout(10, 1), 4, tt) + (size_t)(2 * (tt + KS - 2) + KS) * 4 * 4;
}
inline size_t gconv_shift18_lds(int tt) { return ((size_t)2 * 2 * gc_layout(18, 1).slab(0, tt) + (size_t)2 * 4 * S18_WLP) * 2; }

// grid of the matrix-core kernels: 1-D in the XCD-aware order (GC_BLOCK_INDEX) unless it would not fit 32 bits or the plain
// grid is asked for
inline void gconv_grid(GconvLaunch& p, int64_t tiles, int group_blocks, int B, bool grid_xyz) {
    const int64_t nb = tiles * group_blocks * B;
    if (nb < (1ll << 31) && tiles < (1ll << 31) && !grid_xyz) {
        p.n_tt = (int)tiles;
        p.n_gb = group_blocks;
        p.grid_x = (unsigned)nb; p.grid_y = p.grid_z = 1;
        return;
    }
    p.n_tt = p.n_gb = 0;
    p.grid_x = (unsigned)tiles; p.grid_y = (unsigned)group_blocks; p.grid_z = (unsigned)B;
}

namespace gconv_plan_detail {

inline GconvLaunch refuse(int why) {
    GconvLaunch p = {};
    p.refusal = why;
    return p;
}
inline GconvLaunch start(const GconvCall& c, int kernel, int cig, int cog, int stride, bool resid, int64_t T_out, int ks) {
    GconvLaunch p = {};
    p.kernel = kernel; p.cig = cig; p.cog = cog; p.stride = stride; p.resid = resid;
    p.block = 256;
    p.T_out = T_out;
    p.prof = resid ? GCP_RES : GCP_S2;
    p.work = 2.0 * (double)c.B * (double)T_out * c.C_out * cig * ks;
    return p;
}
// a [gb groups] x [tt output steps] tile per workgroup on the plain (time tile, group block, item) grid: the VALU kernels
inline GconvLaunch tiled(const GconvCall& c, int kernel, int cig, int cog, int stride, int gb, int tt, bool resid, int64_t T_out, int ks) {
    GconvLaunch p = start(c, kernel, cig, cog, stride, resid, T_out, ks);
    p.gb = gb; p.tt = tt;
    p.grid_x = (unsigned)cdiv(T_out, tt); p.grid_y = (unsigned)(c.groups / gb); p.grid_z = (unsigned)c.B;
    p.lds = gconv_valu_lds(cig, gb, tt, stride, ks);
    p.lds_reserve = kernel == GCK_K_TILED ? gconv_valu_lds(cig, gb, tt, stride, TAL_GCONV_MAX_K) : p.lds;
    return p;
}
// one thread per output element (any per-group width)
inline GconvLaunch per_element(const GconvCall& c, int kernel, int stride, bool resid, int64_t T_out, int ks) {
    GconvLaunch p = start(c, kernel, c.C_in / c.groups, c.C_out / c.groups, stride, resid, T_out, ks);
    p.grid_x = (unsigned)cdiv((int64_t)c.B * T_out * c.C_out, 256); p.grid_y = p.grid_z = 1;
    if (kernel == GCK_VALU_GENERIC) p.prof = GCP_NONE;
    return p;
}
// the 1 -> 10 kernels: 20 groups per workgroup, tt_long-step tiles; short inputs (a 30-second clip is 6 tiles of 256 steps x 4
// group blocks = 24 workgroups, 42 us) take 32-step tiles so that the launch covers the chip (a lane walks its tile's time
// steps one after the other)
inline GconvLaunch c1(const GconvCall& c, int kernel, int tt_long, int64_t T_out, int ks) {
    const bool small = cdiv(T_out, tt_long) * (c.groups / 20) * c.B < 256;
    GconvLaunch p = tiled(c, kernel, 1, 10, 2, 20, small ? 32 : tt_long, false, T_out, ks);
    p.ysplit = c.has_y_split;
    p.lds = p.lds_reserve = 0;      // gconv_s2_c1_kernel's slab is static
    if (kernel == GCK_K_C1) p.lds = gconv_k_c1_lds(p.tt, ks), p.lds_reserve = gconv_k_c1_lds(p.tt, TAL_GCONV_MAX_K);
    return p;
}
// gconv_mfma_kernel; x_split: the input is in the split form; no y with y_split: only the split form of the output is written
inline GconvLaunch mfma(const GconvCall& c, int cig, int cog, int stride, bool resid, int gb, int tt, int64_t T_out) {
    if (c.has_y_split && c.C_out % 32 != 0) return refuse(GR_SPLIT_OUT_C);
    // (the split-input slab load moves 4-channel pieces that must not straddle a 32-channel block: the workgroup's first channel,
    //  g0 * CIG with g0 a multiple of GB, has to be a multiple of 4)
    if (c.x_split && !(c.C_in % 32 == 0 && (cig * gb) % 4 == 0)) return refuse(GR_SPLIT_IN_C);
    GconvLaunch p = start(c, GCK_MFMA, cig, cog, stride, resid, T_out, KS);
    p.gb = gb; p.tt = tt;
    p.split = c.has_y ? (c.has_y_split ? 1 : 0) : 2;
    p.xsplit = c.x_split;
    p.lds = p.lds_reserve = gconv_mfma_lds(gc_layout(cig, stride), gb, tt);
    gconv_grid(p, cdiv(T_out, tt), c.groups / gb, c.B, c.o.grid_xyz != 0);
    return p;
}

inline GconvLaunch plan_s2(const GconvCall& c) {
    if (c.has_in_mean && !gconv_c1_ok(c.C_in, c.C_out, c.groups, c.x_lo, c.o.c1_generic != 0, false, true)) return refuse(GR_NO_FOLD_KERNEL);
    if (c.has_y_split && !gconv_c1_ok(c.C_in, c.C_out, c.groups, c.x_lo, c.o.c1_generic != 0, true, false)) return refuse(GR_NO_SPLIT_KERNEL);
    if (!(c.groups > 0 && c.C_in % c.groups == 0 && c.C_out % c.groups == 0)) return refuse(GR_GROUPS);
    if (!(c.B > 0 && c.T_in >= KS)) return refuse(GR_SHAPE);
    const int64_t T_out = (c.T_in - KS) / 2 + 1;
    const int cig = c.C_in / c.groups, cog = c.C_out / c.groups;
    // channel-major lanes: coalesced 256-byte stores (0.29 -> 0.16 ms on the 1-hour shape)
    if (gconv_c1_ok(c.C_in, c.C_out, c.groups, c.x_lo, c.o.c1_generic != 0, c.has_y_split, c.has_in_mean)) return c1(c, GCK_C1, 256, T_out, KS);
    if (cig == 1 && cog == 10 && c.groups % 16 == 0) return tiled(c, GCK_VALU_TILED, 1, 10, 2, 16, 128, false, T_out, KS);
    // Measured on the 1-hour shapes (TFLOP/s): 10->14: 4 groups x 128 outputs 73, 2 x 128 72, 2 x 256 67;
    // 14->18: 2 x 128 75 (31 KB slab, 5 workgroups / CU), 4 x 128 53 (62 KB, 2 / CU), 2 x 256 46.
    // (De-interleaving the slab into even / odd time steps, which removes the 2-way bank conflict of the
    //  stride-2 tap reads, changed nothing: the LDS reads are not the limiter.)
    if (cig == 10 && cog == 14 && c.groups % 4 == 0) return tiled(c, GCK_VALU_TILED, 10, 14, 2, 4, 128, false, T_out, KS);
    if (cig == 14 && cog == 18 && c.groups % 2 == 0) return tiled(c, GCK_VALU_TILED, 14, 18, 2, 2, 128, false, T_out, KS);
    return per_element(c, GCK_VALU_GENERIC, 2, false, T_out, KS);
}

inline GconvLaunch plan_res(const GconvCall& c) {
    if (!(c.groups > 0 && c.C_out % c.groups == 0)) return refuse(GR_GROUPS);
    if (!(c.B > 0 && c.T_in > 0)) return refuse(GR_SHAPE);
    const int cg = c.C_out / c.groups;
    // 2 groups x 256 time steps per workgroup (2 waves per group): 22-40 KB slabs, 4+ workgroups
    // per CU.  Measured on the 1-hour shapes: 66 / 85 / 85 TFLOP/s vs 61 / 67 / 70 with 4 groups.
    if ((cg == 10 || cg == 14 || cg == 18) && c.groups % 2 == 0) return tiled(c, GCK_VALU_TILED, cg, cg, 1, 2, 256, true, c.T_in, KS);
    return per_element(c, GCK_VALU_GENERIC, 1, true, c.T_in, KS);
}

inline GconvLaunch plan_res_f16x3(const GconvCall& c) {
    const int C = c.C_out;
    if (!gconv_has_mfma(C, C, c.groups, 1)) return refuse(GR_NO_MFMA_KERNEL);
    if (!(c.B > 0 && c.T_in > 0)) return refuse(GR_SHAPE);
    if (c.has_y_split && C % 32 != 0) return refuse(GR_SPLIT_C);
    if (!((c.x_lo & 15) == 0 && C % 4 == 0)) return refuse(GR_X_ALIGN);
    if (!gconv_f16x3_fits(c.T_in, C)) return refuse(GR_TOO_LARGE);
    const int64_t T = c.T_in;
    const int cg = C / c.groups, gb = cg == 18 ? 2 : 4;
    const bool shortt = gconv_short_tiles(T, 256, c.groups / gb, c.B, c.o.short_below, c.cus);
    if (cg == 18 && c.x_split && !c.has_y && c.has_y_split && GC_P18 == 20 && GC_KPERM && !c.o.no_shift18) {
        // the product path of the last stage: split form in and out -> the time-shift-packed kernel
        GconvLaunch p = start(c, GCK_SHIFT18, 18, 18, 1, true, T, KS);
        p.gb = 2; p.tt = shortt ? 64 : 256;
        p.split = 2; p.xsplit = true;
        p.lds = p.lds_reserve = gconv_shift18_lds(p.tt);
        gconv_grid(p, cdiv(T, p.tt), c.groups / 2, c.B, c.o.grid_xyz != 0);
        p.nb_total = p.n_tt > 0 ? (int)p.grid_x : 0;
        return p;
    }
    // Long inputs, 14 channels per group: 128-step tiles (38 KB of LDS: four workgroups per CU instead of two at 71 KB) -- the halo grows
    // from 8 to 16 % of the rows filled, but twice the workgroups overlap their dependent phases: 0.317 -> 0.298 ms on the 1-hour shape,
    // 0.220 -> 0.200 on eight 5-minute segments (profiles/r6_gconv_tile_lengths.txt).  10 channels per group (53 KB: three per CU
    // already) lose 9 % with 128 steps and stay at 256; 64-step tiles lose everywhere on long inputs.  Same chain of MFMAs per output:
    // results do not depend on the tile length.  Option gconv_long_tt: 256 / 128 force one length for both widths.
    const bool tt128 = (c.o.long_tt == 128 && cg == 10) || (c.o.long_tt != 256 && cg == 14);
    return mfma(c, cg, cg, 1, true, gb, shortt ? 64 : tt128 ? 128 : 256, T);
}

inline GconvLaunch plan_s2_f16x3(const GconvCall& c) {
    if (!gconv_has_mfma(c.C_in, c.C_out, c.groups, 2)) return refuse(GR_NO_MFMA_KERNEL);
    if (!(c.B > 0 && c.T_in >= KS)) return refuse(GR_SHAPE);
    if (!((c.x_lo & 15) == 0 && c.C_in % 4 == 0)) return refuse(GR_X_ALIGN);
    if (!gconv_f16x3_fits(c.T_in, c.C_in)) return refuse(GR_TOO_LARGE);
    const int64_t T_out = (c.T_in - KS) / 2 + 1;
    const int cig = c.C_in / c.groups, gb = cig == 10 ? 4 : 2;
    const bool shortt = gconv_short_tiles(T_out, 128, c.groups / gb, c.B, c.o.short_below, c.cus);
    return mfma(c, cig, cig + 4, 2, false, gb, shortt ? 64 : 128, T_out);
}

// The first resize conv (1 mel bin -> 10 channels per group) and the first TDSBlock conv of the stage as ONE launch (FROMC1):
// mel [B][T_mel][groups] -> y_split [B][T1][10 groups] in the split form, T1 = (T_mel - 21) / 2 + 1.
inline GconvLaunch plan_c1_res(const GconvCall& c) {
    if (!(c.B > 0 && c.T_in >= KS && gconv_c1_res_fusable(c.C_in, c.C_out, c.groups, c.x_lo))) return refuse(GR_SHAPE);
    const int64_t T1 = (c.T_in - KS) / 2 + 1;
    if (!gconv_f16x3_fits(T1, c.C_out)) return refuse(GR_TOO_LARGE);
    GconvLaunch p = start(c, GCK_C1_RES, 10, 10, 1, true, T1, KS);
    p.gb = 4; p.tt = gconv_short_tiles(T1, 256, c.groups / 4, c.B, c.o.short_below, c.cus) ? 64 : 256;
    p.split = 2; p.xsplit = true;
    p.work = 2.0 * (double)c.B * (double)T1 * c.C_out * (10 + 1) * KS;
    p.lds = p.lds_reserve = gconv_c1_res_lds(p.tt);
    gconv_grid(p, cdiv(T1, p.tt), c.groups / 4, c.B, c.o.grid_xyz != 0);
    return p;
}

inline GconvLaunch plan_s2_k(const GconvCall& c) {
    if (!(c.ks >= 1 && c.ks <= TAL_GCONV_MAX_K)) return refuse(GR_KSIZE);
    if (!(c.groups > 0 && c.C_in % c.groups == 0 && c.C_out % c.groups == 0)) return refuse(GR_GROUPS);
    if (!(c.B > 0 && c.T_in >= c.ks)) return refuse(GR_SHAPE);
    const int64_t T_out = (c.T_in - c.ks) / 2 + 1;
    const int cig = c.C_in / c.groups, cog = c.C_out / c.groups;
    const bool vec = c.C_in % 4 == 0 && (c.x_lo & 15) == 0;
    if (cig == 1 && cog == 10 && c.groups % 20 == 0 && vec) return c1(c, GCK_K_C1, 128, T_out, c.ks);
    if (cig == 10 && cog == 14 && c.groups % 4 == 0 && vec) return tiled(c, GCK_K_TILED, 10, 14, 2, 4, 128, false, T_out, c.ks);
    if (cig == 14 && cog == 18 && c.groups % 2 == 0 && vec) return tiled(c, GCK_K_TILED, 14, 18, 2, 2, 128, false, T_out, c.ks);
    return per_element(c, GCK_K_ANY, 2, false, T_out, c.ks);
}

inline GconvLaunch plan_res_k(const GconvCall& c) {
    if (!(c.ks >= 1 && c.ks <= TAL_GCONV_MAX_K && c.ks % 2 == 1)) return refuse(GR_KSIZE);
    if (!(c.groups > 0 && c.C_out % c.groups == 0)) return refuse(GR_GROUPS);
    if (!(c.B > 0 && c.T_in > 0)) return refuse(GR_SHAPE);
    const int cg = c.C_out / c.groups;
    const bool vec = c.C_out % 4 == 0 && (c.x_lo & 15) == 0 && c.groups % 2 == 0;
    if ((cg == 10 || cg == 14 || cg == 18) && vec) return tiled(c, GCK_K_TILED, cg, cg, 1, 2, 256, true, c.T_in, c.ks);
    return per_element(c, GCK_K_ANY, 1, true, c.T_in, c.ks);
}

}  // namespace gconv_plan_detail

inline GconvLaunch gconv_plan(const GconvCall& c) {
    using namespace gconv_plan_detail;
    switch (c.entry) {
        case GE_S2: return plan_s2(c);
        case GE_RES: return plan_res(c);
        case GE_S2_F16X3: return plan_s2_f16x3(c);
        case GE_RES_F16X3: return plan_res_f16x3(c);
        case GE_C1_RES: return plan_c1_res(c);
        case GE_S2_K: return plan_s2_k(c);
        default: return plan_res_k(c);
    }
}

// the message of a refusal, as the entry points have always worded it (callers and tests/test_abi.py read these texts)
inline void gconv_refusal_text(const GconvCall& c, int why, char* buf, size_t n) {
    const long long T = (long long)c.T_in;
    switch (c.entry * 100 + why) {
        case GE_S2 * 100 + GR_NO_FOLD_KERNEL: snprintf(buf, n, "tal_gconv_s2_fwd: no mean-folding kernel for this shape"); break;
        case GE_S2 * 100 + GR_NO_SPLIT_KERNEL: snprintf(buf, n, "tal_gconv_s2_fwd: no split-output kernel for this shape"); break;
        case GE_S2 * 100 + GR_GROUPS: snprintf(buf, n, "tal_gconv_s2_fwd: channels %d->%d not divisible by groups %d", c.C_in, c.C_out, c.groups); break;
        case GE_S2 * 100 + GR_SHAPE: snprintf(buf, n, "tal_gconv_s2_fwd: T_in=%lld shorter than the kernel", T); break;
        case GE_RES * 100 + GR_GROUPS: snprintf(buf, n, "tal_gconv_res_fwd: C=%d not divisible by groups %d", c.C_out, c.groups); break;
        case GE_RES * 100 + GR_SHAPE: snprintf(buf, n, "tal_gconv_res_fwd: bad shape"); break;
        case GE_RES_F16X3 * 100 + GR_NO_MFMA_KERNEL: snprintf(buf, n, "tal_gconv_res_f16x3_fwd: no fp16x3 kernel for C=%d groups=%d", c.C_out, c.groups); break;
        case GE_RES_F16X3 * 100 + GR_SHAPE: snprintf(buf, n, "tal_gconv_res_f16x3_fwd: bad shape"); break;
        case GE_RES_F16X3 * 100 + GR_SPLIT_C: snprintf(buf, n, "tal_gconv_res_f16x3_fwd: the split output needs C %% 32 == 0 (C=%d)", c.C_out); break;
        case GE_RES_F16X3 * 100 + GR_X_ALIGN: snprintf(buf, n, "tal_gconv_res_f16x3_fwd: x must be 16-byte aligned"); break;
        case GE_RES_F16X3 * 100 + GR_TOO_LARGE: snprintf(buf, n, "tal_gconv_res_f16x3_fwd: one batch item must stay below 2 GiB (T=%lld, C=%d)", T, c.C_out); break;
        case GE_S2_F16X3 * 100 + GR_NO_MFMA_KERNEL:
            snprintf(buf, n, "tal_gconv_s2_f16x3_fwd: no fp16x3 kernel for %d -> %d channels, groups=%d", c.C_in, c.C_out, c.groups);
            break;
        case GE_S2_F16X3 * 100 + GR_SHAPE: snprintf(buf, n, "tal_gconv_s2_f16x3_fwd: T_in=%lld shorter than the kernel", T); break;
        case GE_S2_F16X3 * 100 + GR_X_ALIGN: snprintf(buf, n, "tal_gconv_s2_f16x3_fwd: x must be 16-byte aligned"); break;
        case GE_S2_F16X3 * 100 + GR_TOO_LARGE: snprintf(buf, n, "tal_gconv_s2_f16x3_fwd: one batch item must stay below 2 GiB (T=%lld, C=%d)", T, c.C_in); break;
        case GE_C1_RES * 100 + GR_SHAPE: snprintf(buf, n, "gconv (resize conv + TDSBlock conv): shape not supported"); break;
        case GE_C1_RES * 100 + GR_TOO_LARGE: snprintf(buf, n, "gconv (resize conv + TDSBlock conv): one batch item must stay below 2 GiB"); break;
        case GE_S2_K * 100 + GR_KSIZE: snprintf(buf, n, "tal_gconv_s2_k_fwd: ksize=%d outside 1..%d", c.ks, TAL_GCONV_MAX_K); break;
        case GE_S2_K * 100 + GR_GROUPS: snprintf(buf, n, "tal_gconv_s2_k_fwd: channels %d->%d not divisible by groups %d", c.C_in, c.C_out, c.groups); break;
        case GE_S2_K * 100 + GR_SHAPE: snprintf(buf, n, "tal_gconv_s2_k_fwd: T_in=%lld shorter than the kernel (k=%d)", T, c.ks); break;
        case GE_RES_K * 100 + GR_KSIZE: snprintf(buf, n, "tal_gconv_res_k_fwd: ksize=%d must be odd and in 1..%d", c.ks, TAL_GCONV_MAX_K); break;
        case GE_RES_K * 100 + GR_GROUPS: snprintf(buf, n, "tal_gconv_res_k_fwd: C=%d not divisible by groups %d", c.C_out, c.groups); break;
        case GE_RES_K * 100 + GR_SHAPE: snprintf(buf, n, "tal_gconv_res_k_fwd: bad shape"); break;
        default:        // the matrix-core kernel's own conditions, whichever entry reached it
            if (why == GR_SPLIT_OUT_C) snprintf(buf, n, "gconv (fp16x3): the split output needs C_out %% 32 == 0");
            else snprintf(buf, n, "gconv (fp16x3): the split input needs C_in %% 32 == 0");
            break;
    }
}

}  // namespace tal
