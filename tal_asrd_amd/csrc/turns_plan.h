// Host arithmetic of the speaker-turn kernels (csrc/turns.hip): tile counts, the workspace layouts of tal_speaker_turns_fwd and
// tal_segment_mean_fwd, and the chunks of a range.  Plain C++ (no HIP types; the device qualifiers are empty off-device), so that
// tests/test_turns_plan_cpu.py can run it under a host compiler's sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define TAL_TURNS_HD __host__ __device__
#else
#define TAL_TURNS_HD
#endif

namespace tal {

constexpr int TURNS_TILE = 256;            // frames (and runs, turns, ranges) per workgroup, one per thread
constexpr int TURNS_MAX_HALF = 31;         // largest half window of the mode filter
constexpr int SEGMEAN_CHUNK = 128;         // rows of a chunk of tal_segment_mean_fwd (TAL_SEGMENT_MEAN_CHUNK)
constexpr int SEGMEAN_MAX_E = 1024;
// every index is an int32 and a tile may reach one tile and a halo past the last frame
constexpr int64_t TURNS_MAX_FRAMES = (int64_t)INT32_MAX - 2 * TURNS_TILE - 2 * TURNS_MAX_HALF;

TAL_TURNS_HD inline int64_t turns_up16(int64_t x) { return (x + 15) & ~(int64_t)15; }
TAL_TURNS_HD inline int64_t turns_tiles(int64_t n) { return (n + TURNS_TILE - 1) / TURNS_TILE; }

// Byte offsets inside the workspace of tal_speaker_turns_fwd (all multiples of 16).  Runs and turns number at most N, so their arrays
// are sized for N; the per-tile arrays for the tiles of N.
struct TurnsLayout {
    int64_t smooth;      // int32 [N]   mode-filtered id of every frame
    int64_t flags;       // uint8 [N]   bit 0: the frame starts a run, bit 1: it starts an item
    int64_t run_start;   // int32 [N]   first frame of every run (absolute)
    int64_t run_label;   // int32 [N]
    int64_t run_first;   // uint8 [N]   the run is the first of its item
    int64_t new_label;   // int32 [N]   label of every run after the minimum-duration pass
    int64_t turn_start;  // int32 [N]   first frame of every turn (absolute)
    int64_t count_a;     // int32 [tiles]  run heads per tile of frames, then their exclusive scan
    int64_t count_b;     // int32 [tiles]  turn heads per tile of runs, then their exclusive scan
    int64_t agg;         // int32 [tiles, 4]  per tile of runs: {max long run, max item-first run, min long run, min next item's first run}
    int64_t ctl;         // int32 [4]   {runs, turns, -, -}
    int64_t end;
};

inline TurnsLayout turns_layout(int64_t N) {
    const int64_t nt = turns_tiles(N);
    TurnsLayout l;
    int64_t o = 0;
    l.smooth = o; o += turns_up16(N * 4);
    l.flags = o; o += turns_up16(N);
    l.run_start = o; o += turns_up16(N * 4);
    l.run_label = o; o += turns_up16(N * 4);
    l.run_first = o; o += turns_up16(N);
    l.new_label = o; o += turns_up16(N * 4);
    l.turn_start = o; o += turns_up16(N * 4);
    l.count_a = o; o += turns_up16(nt * 4);
    l.count_b = o; o += turns_up16(nt * 4);
    l.agg = o; o += nt * 16;
    l.ctl = o; o += 16;
    l.end = o;
    return l;
}

// offsets [B + 1] of a call: ascending from 0
inline bool turns_offsets_ok(const int64_t* off, int64_t B, int64_t* N) {
    if (B < 0 || !off || off[0] != 0) return false;
    for (int64_t b = 0; b < B; ++b)
        if (off[b + 1] < off[b]) return false;
    if (off[B] > TURNS_MAX_FRAMES) return false;
    *N = off[B];
    return true;
}

// ---- segment mean: a range [a, b) is cut into chunks of SEGMEAN_CHUNK rows counted from a ----
TAL_TURNS_HD inline int64_t segmean_chunks(int64_t a, int64_t b) { return b > a ? (b - a + SEGMEAN_CHUNK - 1) / SEGMEAN_CHUNK : 0; }
// the most chunks G ranges that cover max_rows rows together can have (every range: at most one partial chunk)
inline int64_t segmean_max_units(int64_t G, int64_t max_rows) { return G + max_rows / SEGMEAN_CHUNK; }

struct SegmeanLayout {
    int64_t units;       // int32 [G]       chunks of every range, then the index of its first chunk
    int64_t tile_sum;    // int32 [tiles(G)] chunks per tile of ranges, then their exclusive scan
    int64_t ctl;         // int32 [4]       {chunks of the call, -, -, -}
    int64_t partial;     // float [max_units, E]
    int64_t end;
};

inline bool segmean_shape_ok(int64_t G, int64_t max_rows, int E) {
    return G >= 0 && max_rows >= 0 && E >= 4 && E <= SEGMEAN_MAX_E && E % 4 == 0 && G <= TURNS_MAX_FRAMES &&
           segmean_max_units(G, max_rows) <= TURNS_MAX_FRAMES;
}

inline SegmeanLayout segmean_layout(int64_t G, int64_t max_rows, int E) {
    SegmeanLayout l;
    int64_t o = 0;
    l.units = o; o += turns_up16(G * 4);
    l.tile_sum = o; o += turns_up16(turns_tiles(G) * 4);
    l.ctl = o; o += 16;
    l.partial = o; o += segmean_max_units(G, max_rows) * (int64_t)E * 4;
    l.end = o;
    return l;
}

}  // namespace tal
