// csrc/turns_plan.h on the host: tile counts, the workspace layouts of tal_speaker_turns_fwd / tal_segment_mean_fwd and the chunks of
// a range, over a grid of sizes up to the int32 bound.  Every region of a layout is WRITTEN (for the sizes that fit in host memory)
// into a buffer of exactly `end` bytes, so an overlap or an overrun is an AddressSanitizer report when the harness is built with
// -fsanitize=address,undefined (tests/test_turns_plan_cpu.py does); the large sizes are checked by arithmetic only.
// Prints the number of combinations; exits non-zero at the first violation.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../tal_asrd_amd/csrc/turns_plan.h"

using namespace tal;

#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            printf("FAILED %s at line %d: N=%lld G=%lld rows=%lld E=%d\n", #cond, __LINE__, \
                   (long long)N, (long long)G, (long long)rows, E);                       \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

// regions (offset, bytes) in order: 16-byte aligned, no overlap, the last one ends at `end`
static bool regions_ok(const std::vector<std::pair<int64_t, int64_t>>& r, int64_t end, bool touch) {
    int64_t pos = 0;
    for (const auto& x : r) {
        if (x.first % 16 || x.first < pos || x.second < 0) return false;
        pos = x.first + x.second;
    }
    if (pos > end || end - pos >= 16) return false;
    if (touch) {
        std::vector<unsigned char> buf((size_t)end);
        std::vector<unsigned char> seen((size_t)end, 0);
        for (const auto& x : r) {
            memset(buf.data() + x.first, 0xab, (size_t)x.second);
            for (int64_t i = 0; i < x.second; ++i)
                if (seen[(size_t)(x.first + i)]++) return false;
        }
    }
    return true;
}

int main() {
    long combos = 0;
    int64_t N = 0, G = 0, rows = 0;
    int E = 0;
    const int64_t Ns[] = {0, 1, 2, 255, 256, 257, 511, 512, 513, 44983, 238912, 1000003, (int64_t)1 << 24, TURNS_MAX_FRAMES};
    for (int64_t n : Ns) {
        N = n;
        const int64_t nt = turns_tiles(N);
        CHECK(N == 0 ? nt == 0 : (nt * TURNS_TILE >= N && (nt - 1) * TURNS_TILE < N));
        CHECK(nt * TURNS_TILE <= INT32_MAX);                                  // the last tile's frame indices are int32
        CHECK((nt - 1) * TURNS_TILE + TURNS_TILE + 2 * TURNS_MAX_HALF + 1 <= INT32_MAX);
        const TurnsLayout L = turns_layout(N);
        CHECK(regions_ok({{L.smooth, N * 4}, {L.flags, N}, {L.run_start, N * 4}, {L.run_label, N * 4}, {L.run_first, N}, {L.new_label, N * 4},
                          {L.turn_start, N * 4}, {L.count_a, nt * 4}, {L.count_b, nt * 4}, {L.agg, nt * 16}, {L.ctl, 16}},
                         L.end, N <= 1000003));
        ++combos;
    }
    // offsets tables
    {
        int64_t n_out = -1;
        const int64_t good[] = {0, 3, 3, 10}, down[] = {0, 5, 4}, late[] = {1, 2}, big[] = {0, TURNS_MAX_FRAMES + 1}, most[] = {0, TURNS_MAX_FRAMES};
        CHECK(turns_offsets_ok(good, 3, &n_out) && n_out == 10);
        CHECK(turns_offsets_ok(good, 0, &n_out) && n_out == 0);
        CHECK(!turns_offsets_ok(down, 2, &n_out) && !turns_offsets_ok(late, 1, &n_out) && !turns_offsets_ok(big, 1, &n_out));
        CHECK(!turns_offsets_ok(nullptr, 1, &n_out) && !turns_offsets_ok(good, -1, &n_out));
        CHECK(turns_offsets_ok(most, 1, &n_out) && n_out == TURNS_MAX_FRAMES);
    }
    // chunks of a range: they tile it from its own start, the last one may be short
    const int64_t starts[] = {0, 1, 127, 128, 1000}, lens[] = {0, 1, 127, 128, 129, 255, 256, 257, 5000, 44983, TURNS_MAX_FRAMES - 1000};
    for (int64_t a : starts)
        for (int64_t len : lens) {
            N = a;
            rows = len;
            const int64_t c = segmean_chunks(a, a + len);
            CHECK(c * SEGMEAN_CHUNK >= len && (c == 0 ? len == 0 : (c - 1) * SEGMEAN_CHUNK < len));
            CHECK(segmean_chunks(a + len, a) == 0);
            CHECK(c <= segmean_max_units(1, len));
            ++combos;
        }
    // G ranges of `rows` rows together never have more chunks than the bound: worst case, rows spread as 1 + whole chunks
    const int64_t Gs[] = {0, 1, 2, 255, 256, 257, 1000, 44983}, Rs[] = {0, 1, 127, 128, 129, 5000, 44983, 238912};
    const int Es[] = {4, 8, 12, 128, 1020, 1024};
    for (int64_t g : Gs)
        for (int64_t r : Rs)
            for (int e : Es) {
                G = g; rows = r; E = e;
                CHECK(segmean_shape_ok(G, rows, E));
                const int64_t units = segmean_max_units(G, rows);
                if (G > 0) {
                    // one row in each range but the first, which takes the rest
                    const int64_t ones = G - 1 < rows ? G - 1 : rows;
                    CHECK(ones + segmean_chunks(0, rows - ones) <= units);
                    // every range one row past a whole number of chunks, as far as the rows go
                    int64_t left = rows, used = 0;
                    for (int64_t i = 0; i < G && left > 0; ++i) {
                        const int64_t take = left < SEGMEAN_CHUNK + 1 ? left : SEGMEAN_CHUNK + 1;
                        used += segmean_chunks(0, take);
                        left -= take;
                    }
                    CHECK(left > 0 || used <= units);
                }
                const SegmeanLayout L = segmean_layout(G, rows, E);
                CHECK(regions_ok({{L.units, G * 4}, {L.tile_sum, turns_tiles(G) * 4}, {L.ctl, 16}, {L.partial, units * E * 4}}, L.end,
                                 units * E * 4 <= (int64_t)64 << 20));
                ++combos;
            }
    G = 1; rows = 0;
    for (int e : {0, 2, 6, 1028, -4}) {
        E = e;
        CHECK(!segmean_shape_ok(1, 10, E));
    }
    E = 4;
    CHECK(!segmean_shape_ok(-1, 10, 4) && !segmean_shape_ok(1, -1, 4) && !segmean_shape_ok(TURNS_MAX_FRAMES, TURNS_MAX_FRAMES * 200, 4));
    printf("combinations %ld\n", combos);
    return 0;
}
