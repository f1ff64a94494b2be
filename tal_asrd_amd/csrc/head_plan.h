// How the streaming heads (csrc/head_stream.h, csrc/soft_embed.hip) cut their work: equal runs of (row block, N tile) units, one
// run per workgroup, and the slots a row's partials take.  Plain C++ (no HIP types; the device qualifiers are empty off-device), so
// that tests/test_head_plan_cpu.py can check the slot bound with a host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

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

}  // namespace tal
