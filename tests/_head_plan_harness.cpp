// csrc/head_plan.h on the host.
//
// Without arguments: the run partition of the streaming heads over a grid of shapes and grid overrides.  Checks what the merge
// kernels rely on (one partial per lane: a row block never meets more than hp <= 16 workgroups) and that block_of is the inverse
// of the runs.  Prints the number of combinations and the largest hp seen; exits non-zero at the first violation.
//
// With the argument "calls": the plan of a call (head_call_plan, head_query_bytes, head_refusal_text) over the sweep of
// tests/_head_call_sweep.h.  Per plan it checks what the kernels and the callers rely on (the partial arrays disjoint, inside the
// needed bytes, aligned for the accesses made to them, as long as the kernels' own indexing makes them; hp within the slots; the
// generic chunk at least one row, its logits inside the workspace; the needed bytes within the query's answer; a refused plan
// names nothing) and prints, for tests/test_head_plan_cpu.py to hold against the record of the entry points before the plan, per
// call a "C" line that names it, an "L" line with the refusal or with what it launches -- the entry points' own few lines around
// the plan are modelled here: the projection in front, the launches of either form, the row chunks -- and a "Q" line with the
// query's answer.  At the end: "A <arm> <count>" per arm of the plan.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../tal_asrd_amd/csrc/head_plan.h"
#include "_head_call_sweep.h"

using namespace tal;

#define CHECK_RUNS(cond)                                                                                                        \
    do {                                                                                                                   \
        if (!(cond)) {                                                                                                     \
            printf("FAILED %s: bn=%d wgs=%d M=%lld S=%d override=%lld grid=%lld hp=%d\n", #cond, bn, wgs, (long long)M, S,   \
                   (long long)ov, (long long)G, p.hp);                                                                    \
            return 1;                                                                                                      \
        }                                                                                                                  \
    } while (0)

static int partition() {
    const int BM = 128, SLOTS = 16, CUS = 256;
    const int widths[] = {128, 64}, per_cu[] = {1, 2};
    const int64_t Ms[] = {1, 5, 127, 128, 129, 300, 1000, 3751, 5000, 44983};
    const int Ss[] = {1, 63, 64, 65, 127, 128, 129, 500, 2007, 6008, 10000, 16008, 40000};
    const int64_t overrides[] = {0, 1, 2, 3, 7, 13, 64, 1000, 100000};
    long combos = 0;
    int worst = 0;
    for (int bn : widths)
        for (int wgs : per_cu)
            for (int64_t M : Ms)
                for (int S : Ss)
                    for (int64_t ov : overrides) {
                        const RunPlan p = head_plan(M, S, BM, bn, SLOTS, wgs, CUS, ov);
                        const int64_t G = p.grid, NT = (S + bn - 1) / bn, MB = (M + BM - 1) / BM, U = MB * NT;
                        CHECK_RUNS(G >= 1);
                        CHECK_RUNS(p.hp >= 1 && p.hp <= SLOTS);
                        const int64_t blocks[] = {0, MB > 1 ? 1 : 0, MB / 2, MB - 1};
                        for (int64_t m : blocks) {
                            const int64_t met = block_of(m * NT + NT - 1, U, G) - block_of(m * NT, U, G) + 1;
                            CHECK_RUNS(met >= 1 && met <= p.hp);
                        }
                        // the runs [b U / G, (b + 1) U / G) are non-empty, adjacent, cover [0, U), and block_of maps both ends of
                        // run b (hence, being monotonic, everything between) back to b
                        int64_t next = 0;
                        for (int64_t b = 0; b < G; ++b) {
                            const int64_t u0 = b * U / G, u1 = (b + 1) * U / G;
                            CHECK_RUNS(u0 == next && u1 > u0);
                            CHECK_RUNS(block_of(u0, U, G) == b && block_of(u1 - 1, U, G) == b);
                            next = u1;
                        }
                        CHECK_RUNS(next == U);
                        worst = p.hp > worst ? p.hp : worst;
                        ++combos;
                    }
    printf("combinations %ld worst_hp %d\n", combos, worst);
    return 0;
}

// ---- the plan of a call ------------------------------------------------------------------------------------------------------------
#define CHECK(cond)                                                 \
    do {                                                            \
        if (!(cond)) {                                              \
            printf("FAILED %s (line %d)\n", #cond, __LINE__);       \
            exit(1);                                                \
        }                                                           \
    } while (0)

using namespace sweep;

enum { A_TOPK_FUSED_K1, A_TOPK_FUSED_K2, A_TOPK_FUSED_K4, A_TOPK_FUSED_K8, A_TOPK_FUSED_K16, A_TOPK_GENERIC, A_XENT_FUSED_64, A_XENT_FUSED_128,
       A_XENT_GENERIC_PACKED, A_XENT_GENERIC_PITCHED, A_SOFT_FUSED_64_SEP, A_SOFT_FUSED_64_W, A_SOFT_FUSED_128_SEP, A_SOFT_FUSED_128_W, A_SOFT_GENERIC,
       A_ROWS, A_PROJECTED_FUSED, A_PROJECTED_GENERIC, A_AUTO_FUSED, A_AUTO_BELOW_THRESHOLD, A_AUTO_NO_FUSED_SHAPE, A_AUTO_OFF_GRID, A_FORCED_FUSED,
       A_FORCED_GENERIC, A_GRID_OVERRIDE, A_GRID_CLAMPED, A_HP_16, A_CHUNK_WHOLE, A_CHUNK_64MIB, A_CHUNK_SHRUNK, A_CHUNK_ONE_ROW, A_TOPK_NEEDS_FULL_CHUNK,
       A_TOPK_WS_OFF_GRID_TAKEN, A_QUERY_TOPK_GENERIC_LARGER, A_QUERY_TOPK_FUSED_LARGER, A_QUERY_TOPK_IGNORES_FORM, A_QUERY_FUSED, A_QUERY_FUSED_FLOOR,
       A_QUERY_GENERIC, A_QUERY_NOTHING, A_NO_ROWS, A_R_FUSED_NEEDS_TOPK, A_R_FUSED_NEEDS_XENT, A_R_FUSED_NEEDS_SOFT, A_R_FUSED_NEEDS_PROJECTED,
       A_R_PROJ_MULT4, A_R_WS_SHORT, A_R_WS_NULL, A_R_WS_SHORT_OF_PROJECTION, A_R_WS_SHORT_BEHIND_PROJECTION, A_R_WS_ALIGN, A_R_DENSE_NEEDS, A_COUNT };
static const char* const arm_names[] = {
    "topk_fused_k1", "topk_fused_k2", "topk_fused_k4", "topk_fused_k8", "topk_fused_k16", "topk_generic", "xent_fused_64", "xent_fused_128",
    "xent_generic_packed", "xent_generic_pitched", "soft_fused_64_sep", "soft_fused_64_w", "soft_fused_128_sep", "soft_fused_128_w", "soft_generic",
    "rows", "projected_fused", "projected_generic", "auto_fused", "auto_below_threshold", "auto_no_fused_shape", "auto_off_grid", "forced_fused",
    "forced_generic", "grid_override", "grid_clamped", "hp_16", "chunk_whole", "chunk_64mib", "chunk_shrunk", "chunk_one_row", "topk_needs_full_chunk",
    "topk_ws_off_grid_taken", "query_topk_generic_larger", "query_topk_fused_larger", "query_topk_ignores_form", "query_fused", "query_fused_floor",
    "query_generic", "query_nothing", "no_rows", "refused_fused_needs_topk", "refused_fused_needs_xent", "refused_fused_needs_soft",
    "refused_fused_needs_projected", "refused_proj_mult4", "refused_ws_short", "refused_ws_null", "refused_ws_short_of_projection",
    "refused_ws_short_behind_projection", "refused_ws_align", "refused_dense_needs"};
static long arms[A_COUNT];

static int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the HeadCall an entry point fills for a case (behind a projection: the head on the projected rows, which lie at the workspace's
// start, and on the workspace behind them)
static HeadCall head_call(const Case& c, bool has_ws, size_t ws_bytes) {
    static const int entry_of[] = {HE_TOPK, HE_XENT_ROWS, HE_LM_XENT, HE_LM_XENT, HE_SOFT_EMBED, HE_SOFT_EMBED, HE_LM_SOFT_EMBED, HE_LM_SOFT_EMBED, HE_SOFT_EMBED_ROWS};
    const bool own_values = c.entry == SE_SOFT || c.entry == SE_SOFT_ROWS;
    HeadCall h = {};
    h.entry = entry_of[c.entry];
    h.M = c.M; h.N = c.N; h.k = c.k;
    h.E = c.entry == SE_SOFT_ROWS ? c.D : c.E;
    h.D = own_values ? c.D : c.E;
    h.ldf = c.entry == SE_SOFT_ROWS ? c.N : c.E + (has_pitch(c.entry) ? c.pitch_extra : 0);
    h.proj_in = is_proj(c.entry) ? c.Dh : 0;
    h.sep = own_values;
    h.feat_lo = is_proj(c.entry) ? c.ws_lo : c.feat_lo;
    h.w_lo = c.entry == SE_SOFT_ROWS ? 0 : c.w_lo;
    h.values_lo = own_values ? c.values_lo : c.w_lo;
    h.ws_lo = has_ws ? c.ws_lo : 0;
    h.workspace_bytes = has_ws ? ws_bytes : 0;
    h.form = c.form; h.grid = c.grid; h.cus = c.cus;
    return h;
}

struct Outcome {
    int rc = 0;
    std::string text;
    Events ev;
    bool planned = false;
    HeadCall h;
    HeadLaunch p;
};

// an entry point from its shape checks on: the projection's share of the workspace, the plan, the launches
static Outcome call_entry(const Case& c, bool has_ws, size_t ws_bytes, bool launches = true) {
    Outcome o;
    if (c.M == 0) return o;
    const char* who = head_entry_name(head_call(c, false, 0).entry);
    const size_t head = is_proj(c.entry) ? lm_proj_bytes(c.M, c.E) : 0;
    if (has_ws ? ws_bytes < head : head > 0) {
        o.rc = TAL_ENOMEM;
        o.text = fmt("%s: workspace %zu < %zu bytes", who, has_ws ? ws_bytes : (size_t)0, head);
        return o;
    }
    const HeadCall h = o.h = head_call(c, has_ws, ws_bytes - (has_ws ? head : 0));
    const HeadLaunch p = o.p = head_call_plan(h);
    o.planned = true;
    if (p.refusal == HR_WS_SHORT && head) {
        o.rc = TAL_ENOMEM;
        o.text = fmt("%s: workspace %zu < %zu bytes", who, ws_bytes, head + p.need);
        return o;
    }
    if (p.refusal) {
        char text[256];
        head_refusal_text(h, p, text, sizeof text);
        o.rc = p.refusal == HR_WS_SHORT ? TAL_ENOMEM : TAL_EINVAL;
        o.text = text;
        return o;
    }
    if (!launches) return o;
    // the operands, as the record's sweep passed them
    const char* h_rows = at<char>(R_FEAT, c.feat_lo);
    const char* w = at<char>(R_W, c.w_lo);
    const char* ws = at<char>(R_WS, c.ws_lo);
    const char* rest = ws + head;
    const char* feat = head ? ws : h_rows;
    const bool lm = h.entry == HE_LM_XENT || h.entry == HE_LM_SOFT_EMBED;
    const char* bias = lm ? nullptr : at<char>(R_BIAS, 0);
    const char* values = h.sep ? at<char>(R_VALUES, c.values_lo) : w;
    const char *target = at<char>(R_TARGET, 0), *out = at<char>(R_OUT, 0), *lse = at<char>(R_LSE, 0), *aux = at<char>(R_AUX, 0);
    Events& ev = o.ev;
    if (head) EV(ev, ev_gemm(h_rows, at<char>(R_PROJ, 0), nullptr, ws, c.M, c.E, c.Dh, (c.Dh + 3) / 4 * 4, c.Dh, c.E));
    const unsigned grid = (unsigned)p.run.grid, rows4 = (unsigned)cdiv64(h.M, 4);
    const int hp = p.run.hp, NT = p.NT, N = h.N, E = h.E, D = h.D, k = h.k, K = p.K;
    const int64_t M = h.M, U = p.U, ldf = h.ldf, pitch = p.pitch;
    const char *p0 = rest + p.off[0], *p1 = rest + p.off[1], *p2 = rest + p.off[2];
    switch (h.entry) {
        case HE_TOPK:
            if (p.fused) {
                EV(ev, ev_stream(TK, fmt("TopkScan<%d>", K), grid, feat, TK, w, bias, M, N, NT, U, p0, p1, p2, hp));
                EV(ev, ev_topk_merge(K, rows4, p0, p1, p2, M, NT, U, p.run.grid, hp, k, out, aux, lse));
                break;
            }
            for_row_chunks(M, p.chunk, [&](int64_t r0, int64_t rows) {
                EV(ev, ev_linear(feat + r0 * E * 4, w, bias, rows, N, E, rest));
                EV(ev, ev_topk_rows(list_len(k), (unsigned)cdiv64(rows, 4), rest, rows, N, k, out + r0 * k * 4, aux + r0 * k * 4, lse + r0 * 4));
                return 0;
            });
            break;
        case HE_XENT_ROWS:
        case HE_LM_XENT:
            if (p.fused) {
                EV(ev, ev_stream(E, "XentScan", grid, feat, ldf, w, bias, M, N, NT, U, target, p0, p1, hp));
                EV(ev, ev_xent_merge(rows4, p0, p1, target, M, NT, U, p.run.grid, hp, out, lse, aux));
                break;
            }
            for_row_chunks(M, p.chunk, [&](int64_t r0, int64_t rows) {
                const char* x = feat + r0 * ldf * 4;
                if (ldf == E) EV(ev, ev_linear(x, w, bias, rows, N, E, rest));
                else EV(ev, ev_gemm(x, w, bias, rest, rows, N, E, ldf, E, N));
                EV(ev, ev_xent_rows((unsigned)cdiv64(rows, 4), rest, rows, N, target + r0 * 8, out + r0 * 4, lse + r0 * 4, aux + r0 * 4));
                return 0;
            });
            break;
        default: {
            if (p.fused) {
                EV(ev, ev_soft(E, h.sep, grid, feat, ldf, w, bias, values, M, N, NT, U, p0, hp));
                EV(ev, ev_soft_merge(rows4, p0, M, E, NT, U, p.run.grid, hp, out, lse));
                break;
            }
            const char *vt = rest, *probs = rest + p.vt;
            const bool have_logits = h.entry == HE_SOFT_EMBED_ROWS;
            EV(ev, ev_transpose((unsigned)cdiv64((int64_t)D * pitch, 256), values, N, D, pitch, vt));
            for_row_chunks(M, p.chunk, [&](int64_t r0, int64_t rows) {
                const char* x = feat + r0 * ldf * 4;
                if (!have_logits) EV(ev, ev_gemm(x, w, bias, probs, rows, N, E, ldf, E, pitch));
                EV(ev, ev_softmax_rows((unsigned)cdiv64(rows, 4), have_logits ? x : probs, have_logits ? ldf : pitch, probs, pitch, rows, N, lse + r0 * 4));
                EV(ev, ev_gemm(probs, vt, nullptr, out + r0 * D * 4, rows, D, (int)pitch, pitch, pitch, D));
                return 0;
            });
        }
    }
    return o;
}

// what the kernels and the callers rely on, and the arms
static void check_plan(const Case& c, const Outcome& o, size_t query) {
    if (c.M == 0) {
        CHECK(query == 0 && !o.planned);
        ++arms[A_NO_ROWS];
        return;
    }
    const bool has_ws = c.ws_mode != WS_NULL;
    if (!o.planned) {       // the workspace does not hold the projected rows
        CHECK(is_proj(c.entry) && o.rc == TAL_ENOMEM);
        ++arms[has_ws ? A_R_WS_SHORT_OF_PROJECTION : A_R_WS_NULL];
        return;
    }
    const HeadCall& h = o.h;
    const HeadLaunch& p = o.p;
    const bool with_values = h.entry >= HE_SOFT_EMBED;      // values^T in front of the generic form's rows
    const bool soft = h.entry == HE_SOFT_EMBED || h.entry == HE_LM_SOFT_EMBED, xent = h.entry == HE_XENT_ROWS || h.entry == HE_LM_XENT;
    const bool shape = h.entry == HE_TOPK ? h.E == 128 : xent ? (h.E == 64 || h.E == 128) : soft ? (h.E == h.D && (h.E == 64 || h.E == 128)) : false;
    const bool on_grid = h.ldf % 4 == 0 && ((h.feat_lo | h.w_lo | (soft ? h.values_lo : 0u)) & 15) == 0;
    const int64_t from_rows = h.entry == HE_TOPK ? 3751 : soft ? 128 : h.E == 64 ? 64 : 3751;
    // the query: never less than the call needs (same options, any alignment)
    CHECK(query > 0);
    if (p.refusal == HR_NONE || p.refusal >= HR_WS_SHORT) CHECK(p.need > 0 && p.need + (is_proj(c.entry) ? lm_proj_bytes(h.M, h.E) : 0) <= query);
    if (p.refusal) {
        // a refused plan names no launch
        CHECK(o.ev.count == 0 && o.rc != 0);
        if (p.refusal < HR_WS_SHORT) CHECK(p.need == 0 && !p.fused && p.chunk == 0 && p.run.grid == 0);
        switch (p.refusal) {
            case HR_FUSED_NEEDS:
                CHECK(h.form == 2 && !(shape && on_grid) && h.entry != HE_SOFT_EMBED_ROWS);
                ++arms[h.proj_in ? A_R_FUSED_NEEDS_PROJECTED : h.entry == HE_TOPK ? A_R_FUSED_NEEDS_TOPK : xent ? A_R_FUSED_NEEDS_XENT : A_R_FUSED_NEEDS_SOFT];
                break;
            case HR_PROJ_MULT4: CHECK(soft && h.proj_in % 4 != 0); ++arms[A_R_PROJ_MULT4]; break;
            case HR_WS_SHORT:
                CHECK(h.workspace_bytes < p.need && o.rc == TAL_ENOMEM);
                ++arms[!has_ws ? A_R_WS_NULL : h.proj_in ? A_R_WS_SHORT_BEHIND_PROJECTION : A_R_WS_SHORT];
                if (h.entry == HE_TOPK && !p.fused && h.workspace_bytes >= (size_t)h.N * 4) ++arms[A_TOPK_NEEDS_FULL_CHUNK];
                break;
            case HR_WS_ALIGN: CHECK(h.entry != HE_TOPK && (h.ws_lo & 15) != 0 && h.workspace_bytes >= p.need); ++arms[A_R_WS_ALIGN]; break;
            default: CHECK(p.refusal == HR_DENSE_NEEDS && soft && !p.fused && (h.E % 4 != 0 || h.ldf % 4 != 0)); ++arms[A_R_DENSE_NEEDS]; break;
        }
        return;
    }
    CHECK(o.rc == 0 && o.ev.count > 0 && h.workspace_bytes >= p.need);
    CHECK(h.entry == HE_TOPK || (h.ws_lo & 15) == 0);
    if (h.entry == HE_TOPK && (h.ws_lo & 15) != 0) ++arms[A_TOPK_WS_OFF_GRID_TAKEN];
    // the form rule
    CHECK(p.fused == (shape && on_grid && (h.form == 2 || (h.form == 0 && h.M >= from_rows))));
    if (h.entry != HE_SOFT_EMBED_ROWS)
        ++arms[h.form == 2 ? A_FORCED_FUSED : h.form != 0 ? A_FORCED_GENERIC : p.fused ? A_AUTO_FUSED : !shape ? A_AUTO_NO_FUSED_SHAPE
               : h.M < from_rows ? A_AUTO_BELOW_THRESHOLD : A_AUTO_OFF_GRID];
    if (h.proj_in) ++arms[p.fused ? A_PROJECTED_FUSED : A_PROJECTED_GENERIC];
    if (p.fused) {
        const int bm = 128, bn = soft ? 64 : 128, per_cu = soft ? 1 : 2;
        const int64_t MB = cdiv64(h.M, bm);
        CHECK(p.NT == cdiv64(h.N, bn) && p.U == MB * p.NT);
        CHECK(p.run.grid >= 1 && p.run.grid <= p.U && p.run.hp >= 1 && p.run.hp <= 16);
        if (h.grid > 0) ++arms[p.run.grid == h.grid ? A_GRID_OVERRIDE : A_GRID_CLAMPED];
        else CHECK(p.run.grid <= (int64_t)per_cu * h.cus);
        if (p.run.hp == 16) ++arms[A_HP_16];
        for (int64_t m : {(int64_t)0, MB / 2, MB - 1})
            CHECK(block_of(m * p.NT + p.NT - 1, p.U, p.run.grid) - block_of(m * p.NT, p.U, p.run.grid) + 1 <= p.run.hp);
        // the partial arrays: as long as the kernels' own indexing makes them (the last element written: row M - 1, slot hp - 1, the second
        // lane half), one behind the other, inside `need`, aligned for the widest access made to them
        const size_t lists = (size_t)h.M * p.run.hp * (soft ? 1 : 2);
        size_t len[3] = {0, 0, 0}, align[3] = {4, 4, 4};
        int npart;
        if (h.entry == HE_TOPK) {
            CHECK(p.K >= h.k && p.K < 2 * h.k && (p.K & (p.K - 1)) == 0 && p.K <= 16);
            npart = 3; len[0] = len[1] = lists * p.K * 4; len[2] = lists * 2 * 4;
            ++arms[p.K == 1 ? A_TOPK_FUSED_K1 : p.K == 2 ? A_TOPK_FUSED_K2 : p.K == 4 ? A_TOPK_FUSED_K4 : p.K == 8 ? A_TOPK_FUSED_K8 : A_TOPK_FUSED_K16];
        } else if (xent) {
            npart = 2; len[0] = lists * 4 * 4; len[1] = lists * 4; align[0] = 16;
            ++arms[h.E == 64 ? A_XENT_FUSED_64 : A_XENT_FUSED_128];
        } else {
            npart = 1; len[0] = lists * (h.D + 4) * 4; align[0] = 16;
            CHECK((h.D + 4) * 4 % 16 == 0);
            ++arms[h.E == 64 ? (h.sep ? A_SOFT_FUSED_64_SEP : A_SOFT_FUSED_64_W) : (h.sep ? A_SOFT_FUSED_128_SEP : A_SOFT_FUSED_128_W)];
        }
        size_t end = 0;
        for (int i = 0; i < npart; ++i) {
            CHECK(p.off[i] >= end && (p.off[i] + h.ws_lo) % align[i] == 0);
            end = p.off[i] + len[i];
        }
        CHECK(end == p.need);
        return;
    }
    // the generic form: whole rows of logits behind values^T, inside the workspace
    const int64_t full = generic_chunk_rows(h.M, p.pitch);
    CHECK(p.pitch == (with_values ? (h.N + 3) / 4 * 4 : h.N) && p.vt == (with_values ? (size_t)h.D * p.pitch * 4 : 0) && p.vt % 16 == 0);
    CHECK(p.chunk >= 1 && p.chunk <= full && p.vt + (size_t)p.chunk * p.pitch * 4 <= h.workspace_bytes);
    CHECK(full == h.M || (size_t)(full + 1) * p.pitch * 4 > ((size_t)64 << 20));
    int64_t covered = 0;
    for_row_chunks(h.M, p.chunk, [&](int64_t r0, int64_t rows) {
        CHECK(r0 == covered && rows >= 1 && rows <= p.chunk);
        covered += rows;
        return 0;
    });
    CHECK(covered == h.M);
    if (p.chunk < full) {
        CHECK(h.entry != HE_TOPK && (size_t)(p.chunk + 1) * p.pitch * 4 > h.workspace_bytes - p.vt);
        ++arms[p.chunk == 1 ? A_CHUNK_ONE_ROW : A_CHUNK_SHRUNK];
    } else {
        ++arms[full == h.M ? A_CHUNK_WHOLE : A_CHUNK_64MIB];
    }
    ++arms[h.entry == HE_TOPK ? A_TOPK_GENERIC : xent ? (h.ldf == h.E ? A_XENT_GENERIC_PACKED : A_XENT_GENERIC_PITCHED) : soft ? A_SOFT_GENERIC : A_ROWS];
}

// the query's arms; `twin`: the answer under the other form options (top-k: the same whatever they say)
static void check_query(const Case& c, size_t query) {
    HeadCall h = head_call(c, false, 0);
    if (c.M == 0) {
        ++arms[A_QUERY_NOTHING];
        return;
    }
    const bool with_values = h.entry >= HE_SOFT_EMBED;
    const size_t pitch = with_values ? ((size_t)h.N + 3) / 4 * 4 : (size_t)h.N, vt = with_values ? (size_t)h.D * pitch * 4 : 0;
    const size_t generic = vt + (size_t)generic_chunk_rows(h.M, (int64_t)pitch) * pitch * 4;
    CHECK(query >= vt + pitch * 4);
    if (h.entry == HE_TOPK) {
        CHECK(query >= generic);
        for (int form : {0, 1, 2}) {
            h.form = form;
            CHECK(head_query_bytes(h) == query);
        }
        ++arms[A_QUERY_TOPK_IGNORES_FORM];
        ++arms[query == generic ? A_QUERY_TOPK_GENERIC_LARGER : A_QUERY_TOPK_FUSED_LARGER];
        return;
    }
    h.form = 1;
    CHECK(head_query_bytes(h) == generic);
    if (query == generic) ++arms[A_QUERY_GENERIC];
    else ++arms[query == vt + pitch * 4 ? A_QUERY_FUSED_FLOOR : A_QUERY_FUSED];
}

static int calls() {
    static_assert(sizeof(arm_names) / sizeof(arm_names[0]) == A_COUNT, "one name per arm");
    long cases = 0;
    run([&](Case c) {
        c.ws_bytes = resolve_ws(c, [&](size_t bytes) {
            const Outcome o = call_entry(c, true, bytes, false);
            const char* lt = o.rc == TAL_ENOMEM ? strstr(o.text.c_str(), " < ") : nullptr;
            return lt ? (size_t)strtoull(lt + 3, nullptr, 10) : (size_t)0;
        });
        print_case(c);
        const Outcome o = call_entry(c, c.ws_mode != WS_NULL, c.ws_bytes);
        print_outcome(o.rc, o.text, o.ev);
        const size_t head = is_proj(c.entry) || c.entry == SE_LM_XENT || c.entry == SE_LM_SOFT ? lm_proj_bytes(c.M, c.E) : 0;
        const size_t answer = head_query_bytes(head_call(c, false, 0)), query = answer ? head + answer : 0;
        print_query(query);
        check_plan(c, o, query);
        check_query(c, answer);
        ++cases;
    });
    for (int a = 0; a < A_COUNT; ++a) printf("A %s %ld\n", arm_names[a], arms[a]);
    printf("cases %ld\n", cases);
    return 0;
}

int main(int argc, char** argv) { return argc > 1 && !strcmp(argv[1], "calls") ? calls() : partition(); }
