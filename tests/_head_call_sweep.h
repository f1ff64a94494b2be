// The calls tests/_head_plan_harness.cpp puts to the streaming heads' plan (csrc/head_plan.h), and how a call and what it launches
// are written down, independent of the plan: the record tests/head_call_parent.txt was made by running the same sweep through the
// entry points as they were before the plan existed, their kernels and dense layers replaced by stubs that write these lines.
//
// Operands are addresses that are never followed: region r starts at r << 40, so a line names a pointer as <region letter>+<bytes>.
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <functional>
#include <initializer_list>
#include <string>
#include <vector>

namespace sweep {

enum Entry {
    SE_TOPK,                // tal_spk_topk_fwd
    SE_XENT_ROWS,           // tal_xent_rows_fwd
    SE_LM_XENT,             // tal_lm_xent_fwd without a projection
    SE_LM_XENT_PROJ,        // ... behind one
    SE_SOFT,                // tal_soft_embed_fwd, values a matrix of its own
    SE_SOFT_W,              // ... values == NULL (values = w)
    SE_LM_SOFT,             // tal_lm_soft_embed_fwd without a projection
    SE_LM_SOFT_PROJ,        // ... behind one
    SE_SOFT_ROWS,           // tal_soft_embed_rows
    SE_COUNT
};
static const char* const entry_names[] = {"topk", "xent_rows", "lm_xent", "lm_xent_proj", "soft", "soft_w", "lm_soft", "lm_soft_proj", "soft_rows"};

inline bool is_xent(int e) { return e == SE_XENT_ROWS || e == SE_LM_XENT || e == SE_LM_XENT_PROJ; }
inline bool is_soft(int e) { return e == SE_SOFT || e == SE_SOFT_W || e == SE_LM_SOFT || e == SE_LM_SOFT_PROJ; }
inline bool is_proj(int e) { return e == SE_LM_XENT_PROJ || e == SE_LM_SOFT_PROJ; }
inline bool has_pitch(int e) { return e != SE_TOPK && e != SE_SOFT_ROWS && !is_proj(e); }       // the features' row pitch is the caller's

enum WsMode { WS_EXACT, WS_ONE_SHORT, WS_ONE_ROW, WS_NULL, WS_AMPLE, WS_TEN_ROWS };

struct Case {
    int entry;
    int64_t M;
    int N, E, D, k;             // E: the head's feature width (LM entries: E0); D: values width (SE_SOFT, SE_SOFT_ROWS; else E)
    int Dh;                     // width of h in front of a projection
    int pitch_extra;            // features' row pitch - width
    unsigned feat_lo, w_lo, values_lo, ws_lo;
    int ws_mode;
    size_t ws_bytes;            // resolved from ws_mode (resolve_ws)
    int form, grid, cus;
};

// ---- addresses ------------------------------------------------------------------------------------------------------------------
enum Region { R_NULL, R_FEAT, R_W, R_VALUES, R_WS, R_BIAS, R_PROJ, R_TARGET, R_OUT, R_LSE, R_AUX };
template <class T>
inline T* at(int region, size_t bytes) { return reinterpret_cast<T*>(((uintptr_t)region << 40) + bytes); }
inline std::string name(const void* p) {
    if (!p) return "0";
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    char buf[40];
    snprintf(buf, sizeof buf, "%c+%llu", "0fwvsbptola"[a >> 40], (unsigned long long)(a & (((uintptr_t)1 << 40) - 1)));
    return buf;
}

// ---- what a call launched: one event per launch, in order ---------------------------------------------------------------------------
// (kept: the first 8, the last and their number -- a one-row workspace means thousands of launches; `make` writes the event out
//  only where it is kept)
struct Events {
    std::vector<std::string> first;
    std::function<std::string()> last;
    long count = 0;
    template <class F>
    void add(F make) {
        if (count < 8) first.push_back(make());
        last = make;
        ++count;
    }
    void clear() { first.clear(); last = nullptr; count = 0; }
};
#define EV(events, text) (events).add([=] { return text; })
inline std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
inline std::string fmt(const char* f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}
#define SN(p) sweep::name(p).c_str()
// a kernel launch: name<template arguments>, grid, then its arguments as the caller formats them
inline std::string ev_kernel(const std::string& kernel, unsigned grid, const std::string& args) { return kernel + fmt("[%u](", grid) + args + ")"; }
// launch_linear (a dense layer on packed rows) and launch_gemm (as launch_linear_ld and the second product fill it)
inline std::string ev_linear(const void* x, const void* w, const void* b, int64_t M, int N, int K, const void* y) {
    return fmt("linear(%s,%s,%s,%lld,%d,%d,%s)", SN(x), SN(w), SN(b), (long long)M, N, K, SN(y));
}
inline std::string ev_gemm(const void* A, const void* W, const void* bias, const void* Y, int64_t M, int N, int K, int64_t lda, int64_t ldw, int64_t ldy) {
    return fmt("gemm(%s,%s,%s,%s,%lld,%d,%d,%lld,%lld,%lld)", SN(A), SN(W), SN(bias), SN(Y), (long long)M, N, K, (long long)lda, (long long)ldw,
               (long long)ldy);
}

// the kernels, each with its arguments in the order of its parameter list
typedef const void* P;
typedef long long LL;
inline std::string ev_stream(int E, const std::string& scan, unsigned grid, P feat, int64_t ldf, P W, P bias, int64_t M, int S, int NT, int64_t U, P a0,
                             P a1, P a2, int HP) {
    return ev_kernel(fmt("head_stream<%d,%s>", E, scan.c_str()), grid,
                     fmt("%s,%lld,%s,%s,%lld,%d,%d,%lld,{%s,%s,%s},%d", SN(feat), (LL)ldf, SN(W), SN(bias), (LL)M, S, NT, (LL)U, SN(a0), SN(a1), SN(a2), HP));
}
inline std::string ev_topk_merge(int K, unsigned grid, P pv, P pi, P pms, int64_t M, int NT, int64_t U, int64_t G, int HP, int k, P ids, P logp, P lse) {
    return ev_kernel(fmt("head_topk_merge<%d>", K), grid,
                     fmt("%s,%s,%s,%lld,%d,%lld,%lld,%d,%d,%s,%s,%s", SN(pv), SN(pi), SN(pms), (LL)M, NT, (LL)U, (LL)G, HP, k, SN(ids), SN(logp), SN(lse)));
}
inline std::string ev_topk_rows(int K, unsigned grid, P x, int64_t M, int N, int k, P ids, P logp, P lse) {
    return ev_kernel(fmt("topk_lse_rows<%d>", K), grid, fmt("%s,%lld,%d,%d,%s,%s,%s", SN(x), (LL)M, N, k, SN(ids), SN(logp), SN(lse)));
}
inline std::string ev_xent_merge(unsigned grid, P pf, P pi, P target, int64_t M, int NT, int64_t U, int64_t G, int HP, P nll, P lse, P top1) {
    return ev_kernel("xent_merge", grid,
                     fmt("%s,%s,%s,%lld,%d,%lld,%lld,%d,%s,%s,%s", SN(pf), SN(pi), SN(target), (LL)M, NT, (LL)U, (LL)G, HP, SN(nll), SN(lse), SN(top1)));
}
inline std::string ev_xent_rows(unsigned grid, P x, int64_t M, int N, P target, P nll, P lse, P top1) {
    return ev_kernel("xent_lse_rows", grid, fmt("%s,%lld,%d,%s,%s,%s,%s", SN(x), (LL)M, N, SN(target), SN(nll), SN(lse), SN(top1)));
}
inline std::string ev_soft(int E, bool sep, unsigned grid, P feat, int64_t ldf, P W, P bias, P V, int64_t M, int S, int NT, int64_t U, P part, int HP) {
    return ev_kernel(fmt("soft_embed<%d,%d>", E, (int)sep), grid,
                     fmt("%s,%lld,%s,%s,%s,%lld,%d,%d,%lld,%s,%d", SN(feat), (LL)ldf, SN(W), SN(bias), SN(V), (LL)M, S, NT, (LL)U, SN(part), HP));
}
inline std::string ev_soft_merge(unsigned grid, P part, int64_t M, int D, int NT, int64_t U, int64_t G, int HP, P out, P lse) {
    return ev_kernel("soft_embed_merge", grid, fmt("%s,%lld,%d,%d,%lld,%lld,%d,%s,%s", SN(part), (LL)M, D, NT, (LL)U, (LL)G, HP, SN(out), SN(lse)));
}
inline std::string ev_softmax_rows(unsigned grid, P x, int64_t ldx, P p, int64_t ldp, int64_t M, int N, P lse) {
    return ev_kernel("softmax_rows", grid, fmt("%s,%lld,%s,%lld,%lld,%d,%s", SN(x), (LL)ldx, SN(p), (LL)ldp, (LL)M, N, SN(lse)));
}
inline std::string ev_transpose(unsigned grid, P values, int N, int D, int64_t ldp, P vt) {
    return ev_kernel("transpose_values", grid, fmt("%s,%d,%d,%lld,%s", SN(values), N, D, (LL)ldp, SN(vt)));
}

// ---- the lines --------------------------------------------------------------------------------------------------------------------
inline void print_case(const Case& c) {
    printf("C %s M=%lld N=%d E=%d D=%d k=%d Dh=%d pitch=+%d lo=%u,%u,%u,%u ws=%d:%zu form=%d grid=%d cus=%d\n", entry_names[c.entry], (long long)c.M, c.N,
           c.E, c.D, c.k, c.Dh, c.pitch_extra, c.feat_lo, c.w_lo, c.values_lo, c.ws_lo, c.ws_mode, c.ws_bytes, c.form, c.grid, c.cus);
}
// rc: the entry's return value; text: its message when rc != 0
inline void print_outcome(int rc, const std::string& text, const Events& ev) {
    if (rc) {
        printf("L refused %d: %s\n", rc, text.c_str());
        return;
    }
    if (!ev.count) {
        printf("L none\n");
        return;
    }
    printf("L");
    for (const std::string& e : ev.first) printf(" %s", e.c_str());
    printf(" n=%ld last=%s\n", ev.count, ev.last().c_str());
}
inline void print_query(size_t bytes) { printf("Q %zu\n", bytes); }

// ---- the workspace of a case --------------------------------------------------------------------------------------------------------
// `rows` rows' worth of the generic form
inline size_t rows_bytes(const Case& c, int rows) {
    const size_t p4 = ((size_t)c.N + 3) / 4 * 4;
    if (is_soft(c.entry) || c.entry == SE_SOFT_ROWS) return (size_t)c.D * p4 * 4 + rows * p4 * 4;
    return (size_t)rows * c.N * 4;
}
// short_by(bytes): the bytes the call says it needs when it refuses a workspace of `bytes` for being short, else 0.  Behind a
// projection the first refusal counts the projected rows alone, the second the whole.
template <class F>
inline size_t resolve_ws(const Case& c, F&& short_by) {
    if (c.ws_mode == WS_NULL) return 0;
    if (c.ws_mode == WS_AMPLE) return (size_t)1 << 38;
    size_t need = short_by((size_t)0), projected = 0;
    if (is_proj(c.entry) && need) {
        projected = need;
        const size_t whole = short_by(need);
        need = whole ? whole : need;
    }
    if (c.ws_mode == WS_ONE_ROW || c.ws_mode == WS_TEN_ROWS) return projected + rows_bytes(c, c.ws_mode == WS_ONE_ROW ? 1 : 10);
    return c.ws_mode == WS_EXACT ? need : need ? need - 1 : 0;
}

// ---- the sweep ----------------------------------------------------------------------------------------------------------------------
static const int64_t ROWS[] = {0, 1, 63, 64, 65, 127, 128, 129, 3750, 3751, 8192, 44983};
static const int WIDTHS[] = {1, 63, 64, 65, 300, 2007, 16008, 40000};
static const int ED[][2] = {{64, 64}, {128, 128}, {64, 128}, {96, 96}, {256, 256}};

inline Case base(int entry, int64_t M, int N, int E, int D) {
    Case c = {};
    c.entry = entry; c.M = M; c.N = N; c.E = E; c.D = D; c.k = 1; c.Dh = 256; c.cus = 256;
    c.ws_mode = WS_EXACT;
    return c;
}

// every entry that takes the pair (E, D): a values width of its own only where values is a matrix of its own
template <class F>
inline void entries(F&& f, int64_t M, int N, int E, int D) {
    for (int e = 0; e < SE_COUNT; ++e) {
        if (E != D && e != SE_SOFT && e != SE_SOFT_ROWS) continue;
        f(base(e, M, N, E, D));
    }
}

template <class F>
inline void run(F&& f) {
    // shapes x forms x CU counts (top-k: every list length too)
    for (int64_t M : ROWS)
        for (int N : WIDTHS)
            for (const auto& ed : ED)
                for (int form : {0, 1, 2})
                    for (int cus : {64, 256, 304})
                        entries([&](Case c) {
                            c.form = form; c.cus = cus;
                            if (c.entry != SE_TOPK) return f(c);
                            for (int k : {1, 2, 3, 5, 8, 16})
                                if (k <= N) c.k = k, f(c);
                        }, M, N, ed[0], ed[1]);
    // grid overrides (a form value outside 0..2 too: it means the generic form everywhere)
    for (int grid : {1, 3, 13, 1000})
        for (int64_t M : ROWS)
            for (int N : WIDTHS)
                for (const auto& ed : ED)
                    for (int form : {0, 2, 3})
                        entries([&](Case c) { c.form = form; c.grid = grid; c.k = N >= 5 ? 5 : 1; f(c); }, M, N, ed[0], ed[1]);
    // the features' row pitch
    for (int extra : {4, 2})
        for (int64_t M : {(int64_t)64, (int64_t)128, (int64_t)3751})
            for (int N : {65, 2007})
                for (const auto& ed : ED)
                    for (int form : {0, 1, 2})
                        entries([&](Case c) {
                            if (!has_pitch(c.entry)) return;
                            if ((c.entry == SE_LM_XENT || c.entry == SE_LM_SOFT) && extra % 4) return;       // (their shape check: pitch in fours)
                            c.form = form; c.pitch_extra = extra;
                            f(c);
                        }, M, N, ed[0], ed[1]);
    // each operand, and the workspace, off the 16-byte grid
    for (int which = 0; which < 4; ++which)
        for (unsigned lo : {4u, 8u})
            for (int64_t M : {(int64_t)63, (int64_t)128, (int64_t)3751})
                for (int N : {64, 300})
                    for (const auto& ed : ED)
                        for (int form : {0, 1, 2})
                            for (int mode : {WS_EXACT, WS_AMPLE})
                                entries([&](Case c) {
                                    c.form = form; c.ws_mode = mode;
                                    (which == 0 ? c.feat_lo : which == 1 ? c.w_lo : which == 2 ? c.values_lo : c.ws_lo) = lo;
                                    f(c);
                                }, M, N, ed[0], ed[1]);
    // the workspace: one byte short, one row's worth, ten rows' worth, none, ample (exactly the needed bytes: everywhere above)
    for (int mode : {WS_ONE_SHORT, WS_ONE_ROW, WS_TEN_ROWS, WS_NULL, WS_AMPLE})
        for (int64_t M : {(int64_t)1, (int64_t)64, (int64_t)129, (int64_t)3751, (int64_t)8192})
            for (int N : {1, 300, 16008})
                for (const auto& ed : ED)
                    for (int form : {0, 1, 2})
                        entries([&](Case c) { c.form = form; c.ws_mode = mode; f(c); }, M, N, ed[0], ed[1]);
    // a projection from a width that is no multiple of 4
    for (int64_t M : {(int64_t)64, (int64_t)3751})
        for (const auto& ed : ED)
            for (int form : {0, 1, 2})
                for (int e : {SE_LM_XENT_PROJ, SE_LM_SOFT_PROJ}) {
                    if (ed[0] != ed[1]) continue;
                    Case c = base(e, M, 2007, ed[0], ed[1]);
                    c.form = form; c.Dh = 510;
                    f(c);
                }
}

}  // namespace sweep
