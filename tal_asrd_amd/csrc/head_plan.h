// What a streaming-head entry point (csrc/head_topk.hip, csrc/xent.hip, csrc/soft_embed.hip) does with a call: how the fused forms
// cut their work -- equal runs of (row block, N tile) units, one run per workgroup, and the slots a row's partials take -- and per
// call the form or the refusal, the bytes it needs, where each partial array lies in the workspace, and the row chunk of the
// generic form, decided from the call's shape, address alignment, workspace size, options and CU count alone.  Plain C++ (no HIP
// types, no pointer dereferenced; the device qualifiers are empty off-device), so that tests/test_head_plan_cpu.py can walk every
// arm with a host compiler.  An entry point checks its arguments, fills a HeadCall, asks for the plan once and acts on it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/tal_asrd.h"

#ifdef __HIPCC__
#define TAL_HOST_DEVICE __host__ __device__
#else
#define TAL_HOST_DEVICE
#endif

namespace tal {

// workgroup whose run [b U / G, (b + 1) U / G) contains unit u
TAL_HOST_DEVICE inline int64_t block_of(int64_t u, int64_t U, int64_t G) {
    int64_t b = u * G / U;
    while ((b + 1) * U / G <= u) ++b;
    while (b * U / G > u) --b;
    return b;
}

// Workgroups of a fused launch and slots per row (a workgroup's slot is its rank among the workgroups of a row block).  A run is
// U / grid units or one more; a row block's NT units then meet at most 1 + ceil((NT - 1) / (U / grid)) runs.  Default: wgs_per_cu
// workgroups per CU (grid_override > 0: that many); runs never shorter than NT / (max_slots - 1) tiles, so hp <= max_slots.
struct RunPlan {
    int64_t grid;
    int hp;
};
inline RunPlan head_plan(int64_t M, int S, int bm, int bn, int max_slots, int wgs_per_cu, int cus, int64_t grid_override) {
    const int64_t nt = (S + bn - 1) / bn, units = (M + bm - 1) / bm * nt, lmin = (nt + max_slots - 2) / (max_slots - 1);
    int64_t g = grid_override > 0 ? grid_override : (int64_t)wgs_per_cu * cus;
    if (g > units) g = units;
    if (units / g < lmin) g = units / lmin;
    const int64_t len = units / g, slots = 1 + (nt - 1 + len - 1) / len;
    return {g, (int)(slots < g ? slots : g)};
}

// the generic forms write the logits of a chunk of rows (row pitch `pitch` floats) into the workspace: 64 MiB worth at most
constexpr size_t GENERIC_WS_MAX = (size_t)64 << 20;
inline int64_t generic_chunk_rows(int64_t M, int64_t pitch) {
    int64_t rows = (int64_t)(GENERIC_WS_MAX / ((size_t)pitch * 4));
    rows = rows < 1 ? 1 : rows;
    return rows < M ? rows : M;
}

// ---- the constants the decisions rest on ----------------------------------------------------------------------------------------
// head_stream_kernel (csrc/head_stream.h: top-k and scoring): rows per block, columns per N tile, most workgroup slots per row
constexpr int HS_BM = 128, HS_BN = 128;
constexpr int HS_SLOTS = 16;
constexpr int TK = 128;             // feature width (K) of the fused top-k form
// soft_embed_kernel (csrc/soft_embed.hip)
constexpr int SBM = 128, SBN = 64;
constexpr int SP_MAX = 16;          // most workgroup slots per row
constexpr int SHDR = 4;             // floats in front of a partial's out[D]: (max, sum, -, -) -- keeps out[] 16-byte aligned

// Rows at and above which auto dispatch (form option 0) takes the fused form.
// Top-k, E = 128: the smallest row count of the sweep in profiles/head_topk.txt at which it measured faster than the generic form
// (2048 rows: generic 0.114 ms, fused 0.126; 3751 rows: 0.225 / 0.176).
constexpr int64_t TOPK_FUSED_FROM_ROWS = 3751;
// Scoring, per feature width.
// E = 64 (the factorised LM head): the fused form measured faster than the generic one at EVERY row count of the sweep in
// profiles/lm_xent.txt, whose smallest is 64 rows ((D, E0, V) = (512, 64, 16008): generic 0.119 ms, fused 0.098; (256, 64, 10000):
// 0.081 / 0.076; at 16,384 rows 2.249 / 0.506 and 1.064 / 0.320).  Below 64 rows nothing was measured, so nothing is assumed.
// E = 128 (the speaker head): TOPK_FUSED_FROM_ROWS, the cross-over of the same skeleton at this width (profiles/head_topk.txt).
// The sweep of THIS kernel (profiles/lm_xent.txt, last table) puts its own cross-over lower -- 256 rows: generic 0.060 ms, fused
// 0.076; 512 rows: 0.073 / 0.064 -- so the constant is on the safe side between 512 and 3,750 rows (the generic form there costs up
// to 0.17 against 0.10 ms at 4,096 rows); lowering it to 512 is a follow-up with its own run.
constexpr int64_t XENT_FUSED_FROM_ROWS_E64 = 64, XENT_FUSED_FROM_ROWS_E128 = 3751;
// Soft embedding.  Rule: the smallest row count of the sweep in profiles/soft_embed.txt from which the fused form measured faster
// than the generic one at EVERY larger row count of the sweep.  It did at every row count of the ladder, whose smallest is 128 rows
// (N = 6008; E = 128: fused 0.086 ms, generic 0.112; E = 64: 0.054 / 0.109; at 16,384 rows 0.480 / 4.087 and 0.275 / 3.965; at the
// 1-hour shape, 44,983 rows, 1.226 / 11.009 and 0.713 / 10.687).  Below 128 rows nothing was measured, so nothing is assumed: the
// generic form.
constexpr int64_t SOFT_FUSED_FROM_ROWS_E64 = 128, SOFT_FUSED_FROM_ROWS_E128 = 128;

inline int list_len(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16; }       // the top-k kernels' list lengths
// the soft embedding's generic form: the probabilities' row pitch (N rounded up to 4) and values^T [D, pitch4(N)] in front of them
inline int64_t pitch4(int N) { return ((int64_t)N + 3) / 4 * 4; }
inline size_t vt_bytes(int N, int D) { return (size_t)D * (size_t)pitch4(N) * 4; }       // (a multiple of 16)
// f(r0, rows) for each [r0, r0 + rows) of M rows, `chunk` at a time; stops at the first non-zero return and hands it on
template <class F>
inline int for_row_chunks(int64_t M, int64_t chunk, F&& f) {
    int rc = 0;
    for (int64_t r0 = 0; r0 < M && !rc; r0 += chunk) rc = f(r0, M - r0 < chunk ? M - r0 : chunk);
    return rc;
}

// ---- the plan of a call -----------------------------------------------------------------------------------------------------------
// tal_spk_topk_fwd, tal_xent_rows_fwd, tal_lm_xent_fwd, tal_soft_embed_fwd, tal_lm_soft_embed_fwd, tal_soft_embed_rows (the generic
// tail alone, on the caller's logits).  Behind an LM projection (proj_in > 0) the head is planned on the projected rows [M, E0], which
// take the head of the workspace (lm_proj_bytes: rounded up to 16 bytes), and on the rest of the workspace.
enum HeadEntry { HE_TOPK, HE_XENT_ROWS, HE_LM_XENT, HE_SOFT_EMBED, HE_LM_SOFT_EMBED, HE_SOFT_EMBED_ROWS };
inline size_t lm_proj_bytes(int64_t M, int E0) { return ((size_t)M * E0 * sizeof(float) + 15) & ~(size_t)15; }

// The facts of a call the decisions rest on.  The entry point has checked the shape and the pointers; M > 0 (the queries: any M).
struct HeadCall {
    int entry;
    int64_t M;
    int N, E, D, k;                 // head width, feature width, values width (soft embedding; else E), list length (top-k; else 1)
    int64_t ldf;                    // row pitch of the features (floats)
    int proj_in;                    // the width of h in front of an LM projection; 0: the head runs on the caller's rows
    bool sep;                       // soft embedding: values is a matrix of its own (not w)
    unsigned feat_lo, w_lo, values_lo, ws_lo;       // the low four address bits of the operands and of the workspace
    size_t workspace_bytes;         // 0 for a NULL workspace
    int form, grid, cus;            // the head's *_form and *_grid options, the CU count
};

// HR_FUSED_NEEDS: form option 2 on a call that cannot take the fused form; HR_PROJ_MULT4 / HR_DENSE_NEEDS: the soft embedding's dense
// layers need widths and pitches in fours; HR_WS_SHORT is TAL_ENOMEM, every other refusal TAL_EINVAL
enum HeadRefusal { HR_NONE, HR_FUSED_NEEDS, HR_PROJ_MULT4, HR_WS_SHORT, HR_WS_ALIGN, HR_DENSE_NEEDS };

struct HeadLaunch {
    int refusal;                    // != HR_NONE: nothing is launched
    bool fused;
    size_t need;                    // bytes of workspace the call needs (filled from HR_WS_SHORT on)
    // fused form: the run partition, N tiles, units, top-k's list length K, and the byte offset of each partial array in the workspace,
    // per row, slot (and lane half: top-k, scoring):   top-k    [M, hp, 2] x  K values | K indices | (max, sum)
    //                                                  scoring  [M, hp, 2] x  (max, sum, best value, target logit) | best index
    //                                                  soft     [M, hp]    x  (max, sum, -, -, out[D])
    RunPlan run;
    int NT, K;
    int64_t U;
    size_t off[3];
    // generic form: values^T in front (soft embedding), then `chunk` rows of logits / probabilities at `pitch` floats
    size_t vt;
    int64_t pitch, chunk;
};

// One rule for all heads: fused iff the shape has a fused kernel, the row pitch is in fours, feat / w (/ values) lie on the 16-byte
// grid, and the form option is 2, or 0 with M at or above the head's threshold.  What the heads do differently ON PURPOSE (callers
// and tests rely on each):            top-k                       scoring                      soft embedding (and _rows)
//   fused shapes                      E = 128                     E = 64, 128                  E = D = 64, 128
//   run partition                     128 x 128 units, 2 per CU   same                         128 x 64 units, 1 per CU (the LDS image)
//   generic form needs at least       the full chunk              one row of logits            values^T + one row
//   generic chunk                     never shrinks               as many rows as the workspace holds (both)
//   workspace off the 16-byte grid    taken (4-byte accesses)     refused                      refused
//   query answers                     max(generic, fused),        the form the shape takes under the options, and never less
//                                     whatever the options say    than the generic form's least (both)
namespace head_plan_detail {

inline bool soft(const HeadCall& c) { return c.entry == HE_SOFT_EMBED || c.entry == HE_LM_SOFT_EMBED; }
inline bool fused_shape(const HeadCall& c) {
    if (c.entry == HE_TOPK) return c.E == TK;
    return c.entry != HE_SOFT_EMBED_ROWS && (c.E == 64 || c.E == 128) && (!soft(c) || c.E == c.D);
}
// the form the dispatch takes BY SHAPE under the options in force (alignment is only known at the call)
inline bool fused_by_shape(const HeadCall& c) {
    const int64_t from = c.entry == HE_TOPK ? TOPK_FUSED_FROM_ROWS
                         : soft(c)          ? (c.E == 64 ? SOFT_FUSED_FROM_ROWS_E64 : SOFT_FUSED_FROM_ROWS_E128)
                                            : (c.E == 64 ? XENT_FUSED_FROM_ROWS_E64 : XENT_FUSED_FROM_ROWS_E128);
    return fused_shape(c) && (c.form == 2 || (c.form == 0 && c.M >= from));
}
inline bool fused_possible(const HeadCall& c) {
    return fused_shape(c) && c.ldf % 4 == 0 && ((c.feat_lo | c.w_lo | (soft(c) ? c.values_lo : 0u)) & 15) == 0;
}
// the fused form's run partition and partial arrays, one behind the other; returns their bytes
inline size_t fused_layout(const HeadCall& c, HeadLaunch& p) {
    const bool s = soft(c);
    p.run = s ? head_plan(c.M, c.N, SBM, SBN, SP_MAX, 1, c.cus, c.grid) : head_plan(c.M, c.N, HS_BM, HS_BN, HS_SLOTS, 2, c.cus, c.grid);
    p.NT = (c.N + (s ? SBN : HS_BN) - 1) / (s ? SBN : HS_BN);
    p.U = (c.M + (s ? SBM : HS_BM) - 1) / (s ? SBM : HS_BM) * p.NT;
    p.K = list_len(c.k);
    const size_t lists = (size_t)c.M * p.run.hp * (s ? 1 : 2);
    const size_t first = c.entry == HE_TOPK ? lists * p.K * 4 : s ? lists * (size_t)(c.D + SHDR) * 4 : lists * 16;
    const size_t second = c.entry == HE_TOPK ? first : s ? 0 : lists * 4, third = c.entry == HE_TOPK ? lists * 8 : 0;
    p.off[0] = 0; p.off[1] = first; p.off[2] = first + second;
    return first + second + third;
}
// the generic form's layout with the full chunk; returns the least bytes it runs on
inline size_t generic_layout(const HeadCall& c, HeadLaunch& p) {
    const bool values = c.entry >= HE_SOFT_EMBED;
    p.vt = values ? vt_bytes(c.N, c.D) : 0;
    p.pitch = values ? pitch4(c.N) : c.N;
    p.chunk = generic_chunk_rows(c.M, p.pitch);
    return p.vt + (size_t)(c.entry == HE_TOPK ? p.chunk : 1) * (size_t)p.pitch * 4;
}

}  // namespace head_plan_detail

inline HeadLaunch head_call_plan(const HeadCall& c) {
    using namespace head_plan_detail;
    HeadLaunch p = {};
    const auto refuse = [&](int why) { p.refusal = why; return p; };
    if (c.form == 2 && c.entry != HE_SOFT_EMBED_ROWS && !fused_possible(c)) return refuse(HR_FUSED_NEEDS);
    if (soft(c) && c.proj_in > 0 && !(c.proj_in % 4 == 0 && c.E % 4 == 0)) return refuse(HR_PROJ_MULT4);
    p.fused = fused_by_shape(c) && fused_possible(c);
    p.need = p.fused ? fused_layout(c, p) : generic_layout(c, p);
    if (c.workspace_bytes < p.need) return refuse(HR_WS_SHORT);
    if (c.entry != HE_TOPK && (c.ws_lo & 15) != 0) return refuse(HR_WS_ALIGN);
    if (p.fused) return p;
    if (soft(c) && !(c.E % 4 == 0 && c.ldf % 4 == 0)) return refuse(HR_DENSE_NEEDS);
    const int64_t fit = (int64_t)((c.workspace_bytes - p.vt) / ((size_t)p.pitch * 4));
    if (c.entry != HE_TOPK && fit < p.chunk) p.chunk = fit;
    return p;
}

// the answer of the *_workspace_bytes queries (the LM entries add lm_proj_bytes); 0 for a shape no call takes
inline size_t head_query_bytes(const HeadCall& c) {
    using namespace head_plan_detail;
    if (c.M <= 0 || c.N <= 0 || c.E <= 0 || c.D <= 0 || c.k < 1 || c.k > TAL_TOPK_MAX) return 0;
    HeadLaunch g = {}, f = {};
    const size_t least = generic_layout(c, g), generic = g.vt + (size_t)g.chunk * (size_t)g.pitch * 4;
    if (c.entry == HE_TOPK ? !fused_shape(c) : !fused_by_shape(c)) return generic;
    const size_t fused = fused_layout(c, f), floor = c.entry == HE_TOPK ? generic : least;
    return fused > floor ? fused : floor;
}

// the message of a refusal, as the entry points have always worded it (callers and the GPU tests read these texts)
inline const char* head_entry_name(int entry) {
    static const char* const names[] = {"tal_spk_topk_fwd",   "tal_xent_rows_fwd",     "tal_lm_xent_fwd",
                                        "tal_soft_embed_fwd", "tal_lm_soft_embed_fwd", "tal_soft_embed_rows"};
    return names[entry];
}
inline void head_refusal_text(const HeadCall& c, const HeadLaunch& p, char* buf, size_t n) {
    const char* who = head_entry_name(c.entry);
    switch (p.refusal) {
        case HR_FUSED_NEEDS:
            if (c.entry == HE_TOPK)
                snprintf(buf, n, "%s: the fused form needs E == %d and 16-byte aligned operands (E=%d)", who, TK, c.E);
            else if (c.proj_in > 0)
                snprintf(buf, n, "%s: the fused form needs E0 == 64 or 128 and 16-byte aligned operands (E0=%d)", who, c.E);
            else if (head_plan_detail::soft(c))
                snprintf(buf, n, "%s: the fused form needs E == D == 64 or 128, a row pitch that is a multiple of 4 and 16-byte aligned operands "
                         "(E=%d, D=%d)", who, c.E, c.D);
            else
                snprintf(buf, n, "%s: the fused form needs E == 64 or 128, a row pitch that is a multiple of 4 and 16-byte aligned operands (E=%d)",
                         who, c.E);
            break;
        case HR_PROJ_MULT4: snprintf(buf, n, "%s: D and E0 must be multiples of 4", who); break;
        case HR_WS_SHORT: snprintf(buf, n, "%s: workspace %zu < %zu bytes", who, c.workspace_bytes, p.need); break;
        case HR_WS_ALIGN: snprintf(buf, n, "%s: the workspace must be 16-byte aligned", who); break;
        default: snprintf(buf, n, "%s: the dense layer needs E and the row pitch to be multiples of 4 (E=%d)", who, c.E); break;
    }
}

}  // namespace tal
