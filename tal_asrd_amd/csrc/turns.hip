// Speaker turns on the device: per-frame speaker ids (SDModel.speaker_ids) -> smoothed who-spoke-when turns with one mean
// feature per turn.  Integers on every decision: each integer output equals the host model of tests/_turns_ref.py exactly.
//
// FRAMES.  ids int32 [N] are the frames of B items back to back, item b = [offsets[b], offsets[b + 1]).  Work is cut into tiles of
// TURNS_TILE = 256 frames (runs, turns, ranges), one per thread of a 256-thread workgroup.
//
// MODE FILTER (turns_mode_kernel, one workgroup per tile of frames).  The tile with a halo of w + 1 frames before and w behind is
// staged in LDS; frame t counts every distinct id of its window [t - w, t + w] CLIPPED TO ITS ITEM (the item comes from a binary
// search of offsets, so a boundary inside a tile is the ordinary case) and keeps the most frequent one -- ties: the centre's own id
// if it is among them, else the smallest.  Thread 0 also filters frame t0 - 1, so that run heads (frame starts an item, or its
// filtered id differs from the previous frame's) are known inside the launch; the launch leaves the head count of every tile.
// The same kernel raises bit 0 of the status word for an id outside [0, num_ids); every later kernel of the call then returns at
// once.  No kernel of this file indexes memory by an id.
//
// COMPACTION = count -> scan -> scatter, three launches each time; the scan of the per-tile counts is ONE workgroup that walks them in
// chunks of 256 with a carry.  No kernel waits for another workgroup: every dependency is stream order.
//   runs:   heads per tile (mode kernel) -> scan -> run_start / run_label / run_first
//   step c: a run shorter than min_frames takes the label of the nearest long run before it in its item, else of the nearest one
//           after it, else keeps its own.  "Nearest long run before" is a prefix max of (r if long else -1); it lies in the same item
//           iff it is >= the prefix max of (r if run r is the first of an item else -1).  "After" is the mirrored suffix min against
//           the suffix min of (r + 1 if run r + 1 is the first of an item).  Plain max / min scans, so no segmented operator:
//           per-tile aggregates -> one-workgroup exclusive scan of the aggregates -> per-tile scan with the carries.
//   turns:  a run starts a turn if it is the first of its item or its new label differs from the previous run's: count -> scan -> scatter.
//   finish: per turn start / end relative to its item (and absolute, the ranges of the segment mean), purity = 0; turn_offsets[b] = the turn that holds frame offsets[b].
//   frames: every frame finds its turn by binary search of the turn starts, writes frame_labels, and counts raw-id matches into
//           purity: LDS counters per tile, then one integer atomic per (tile, turn) -- integers, so the order cannot matter.
//
// SEGMENT MEAN (tal_segment_mean_fwd).  Range g = [a, b) of feat rows is cut into chunks of SEGMEAN_CHUNK = 128 rows counted from a.
// count (chunks per range) -> scan -> first chunk of every range; then a grid-stride loop over all chunks: the workgroup sums one chunk
// with E / 4 column threads (16-byte loads) x 256 / (E / 4) row slots, slot j adding rows j, j + slots, ... in order and slot 0 adding
// the slots' sums in slot order; last one thread per 4 columns adds a range's chunk sums in chunk order and divides.  The order of
// every addition is fixed by (a, b, E) alone: no float atomics, the same bits for any grid and any company of other ranges.
#include "common.h"
#include "turns_plan.h"

namespace tal {

namespace {

constexpr int TILE = TURNS_TILE, MAXW = TURNS_MAX_HALF;
constexpr int BIG = INT32_MAX;
static_assert(TILE == 256, "one frame per thread of four waves");
static_assert(MAXW == TAL_TURNS_MAX_HALF && SEGMEAN_CHUNK == TAL_SEGMENT_MEAN_CHUNK, "turns_plan.h and include/tal_asrd.h must agree");

struct OpSum { __device__ int operator()(int a, int b) const { const int64_t s = (int64_t)a + b; return s > BIG ? BIG : (int)s; } };      // (saturating: non-negative addends)
struct OpMax { __device__ int operator()(int a, int b) const { return a > b ? a : b; } };
struct OpMin { __device__ int operator()(int a, int b) const { return a < b ? a : b; } };

struct ScanLds {
    int wtot[4];
    int tmp[TILE];
};

// inclusive scan over the 256 threads of the workgroup (every thread calls)
template <class Op>
__device__ __forceinline__ int block_scan(int v, Op op, int ident, ScanLds& l) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int n = __shfl_up(v, off, 64);
        if (lane >= off) v = op(n, v);
    }
    __syncthreads();
    if (lane == 63) l.wtot[wv] = v;
    __syncthreads();
    int add = ident;
    for (int q = 0; q < wv; ++q) add = op(add, l.wtot[q]);
    return op(add, v);
}

// exclusive scan; `total` = the value over all 256 threads
template <class Op>
__device__ __forceinline__ int block_scan_excl(int v, Op op, int ident, ScanLds& l, int& total) {
    const int inc = block_scan(v, op, ident, l);
    l.tmp[threadIdx.x] = inc;
    __syncthreads();
    const int ex = threadIdx.x ? l.tmp[threadIdx.x - 1] : ident;
    total = l.tmp[TILE - 1];
    __syncthreads();
    return ex;
}

__device__ __forceinline__ int block_count(bool p, int* word) {
    if (threadIdx.x == 0) *word = 0;
    __syncthreads();
    const unsigned long long b = __ballot(p);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(word, __popcll(b));
    __syncthreads();
    return *word;
}

// the largest b in [0, B) with off[b] <= t (0 <= t < off[B], off[0] == 0): the item that owns frame t
__device__ __forceinline__ int item_of(const int64_t* __restrict__ off, int B, int t) {
    int a = 0, b = B;
    while (b - a > 1) {
        const int mid = a + ((b - a) >> 1);
        if (off[mid] <= t) a = mid; else b = mid;
    }
    return a;
}

// number of entries of the ascending v[0 .. n) that are <= t, minus one: the turn that holds frame t (v[0] <= t)
__device__ __forceinline__ int last_le(const int32_t* __restrict__ v, int n, int t) {
    int a = 0, b = n;
    while (b - a > 1) {
        const int mid = a + ((b - a) >> 1);
        if (v[mid] <= t) a = mid; else b = mid;
    }
    return a;
}

// mode of the window of frame t inside its item [lo, hi); sm[p - base] holds ids[p]
__device__ __forceinline__ int mode_at(const int* sm, int base, int t, int lo, int hi, int w) {
    const int a = (t - w > lo ? t - w : lo) - base, b = (t + w < hi - 1 ? t + w : hi - 1) - base;
    const int c = sm[t - base];
    int cc = 0;
    for (int q = a; q <= b; ++q) cc += sm[q] == c;
    if (2 * cc > b - a + 1) return c;      // (an absolute majority)
    int best = c, bestc = cc;
    bool centre = true;
    for (int p = a; p <= b; ++p) {
        const int v = sm[p];
        if (v == c || (p > a && v == sm[p - 1])) continue;      // (the same candidate as the position before: the same count)
        int n = 0;
        for (int q = a; q <= b; ++q) n += sm[q] == v;
        if (n > bestc || (n == bestc && !centre && v < best)) {
            best = v;
            bestc = n;
            centre = false;
        }
    }
    return best;
}

__global__ __launch_bounds__(TILE) void turns_mode_kernel(const int32_t* __restrict__ ids, const int64_t* __restrict__ off, int B, int N,
                                                         int num_ids, int w, int32_t* __restrict__ smooth, uint8_t* __restrict__ flags,
                                                         int32_t* __restrict__ count, int32_t* status) {
    __shared__ int sm[TILE + 2 * MAXW + 1];
    __shared__ int res[TILE + 1];
    __shared__ int heads;
    const int i = threadIdx.x;
    const int t0 = blockIdx.x * TILE, base = t0 - w - 1, span = TILE + 2 * w + 1;
    for (int j = i; j < span; j += TILE) {
        const int64_t p = (int64_t)base + j;
        sm[j] = p >= 0 && p < N ? ids[p] : 0;
    }
    __syncthreads();
    const int t = t0 + i;
    const bool live = t < N;
    int lo = 0, s = 0;
    if (live) {
        const int b = item_of(off, B, t);
        lo = (int)off[b];
        const int hi = (int)off[b + 1];
        const int c = sm[t - base];
        if (c < 0 || c >= num_ids) atomicOr(status, TAL_TURNS_STATUS_BAD_ID);
        s = mode_at(sm, base, t, lo, hi, w);
        res[i + 1] = s;
        if (i == 0 && t > lo) res[0] = mode_at(sm, base, t - 1, lo, hi, w);
    }
    __syncthreads();
    bool head = false;
    if (live) {
        head = t == lo || res[i] != s;
        smooth[t] = s;
        flags[t] = (uint8_t)((head ? 1 : 0) | (t == lo ? 2 : 0));
    }
    const int n = block_count(head, &heads);
    if (i == 0) count[blockIdx.x] = n;
}

// a[0 .. n) -> its exclusive prefix sums in place, *total = the sum (one workgroup)
__global__ __launch_bounds__(TILE) void turns_scan_sum_kernel(int32_t* a, int n, int32_t* total, const int32_t* status) {
    __shared__ ScanLds l;
    if (status && *status) return;
    int carry = 0;
    for (int c0 = 0; c0 < n; c0 += TILE) {
        const int idx = c0 + (int)threadIdx.x;
        int tot;
        const int ex = block_scan_excl(idx < n ? a[idx] : 0, OpSum(), 0, l, tot);
        if (idx < n) a[idx] = OpSum()(carry, ex);
        carry = OpSum()(carry, tot);
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(TILE) void turns_runs_scatter_kernel(const int32_t* __restrict__ smooth, const uint8_t* __restrict__ flags,
                                                                 const int32_t* __restrict__ count, int N, int32_t* __restrict__ run_start,
                                                                 int32_t* __restrict__ run_label, uint8_t* __restrict__ run_first,
                                                                 const int32_t* status) {
    __shared__ ScanLds l;
    if (*status) return;
    const int t = blockIdx.x * TILE + threadIdx.x;
    const int f = t < N ? flags[t] : 0;
    const int inc = block_scan(f & 1, OpSum(), 0, l);
    if (f & 1) {
        const int r = count[blockIdx.x] + inc - 1;
        run_start[r] = t;
        run_label[r] = smooth[t];
        run_first[r] = (uint8_t)(f >> 1);
    }
}

// For run r = base + threadIdx.x of a tile of runs, over the runs of the TILE only: pl = the last long run <= r (-1: none),
// pf = the last run <= r that is the first of an item, nl = the first long run >= r (BIG: none), nf = the first run > r that is the
// first of an item.  The backward scans run on the mirrored index and come back through LDS.
struct RunScan {
    int pl, pf, nl, nf, len;
};
__device__ __forceinline__ RunScan run_scans(int base, int R, int N, int m, const int32_t* __restrict__ run_start,
                                            const uint8_t* __restrict__ run_first, ScanLds& l, int (*xch)[TILE]) {
    const int i = threadIdx.x;
    RunScan o;
    auto length = [&](int r) { return r < R ? (r + 1 < R ? run_start[r + 1] : N) - run_start[r] : 0; };
    const int r = base + i;
    o.len = length(r);
    o.pl = block_scan(r < R && o.len >= m ? r : -1, OpMax(), -1, l);
    o.pf = block_scan(r < R && run_first[r] ? r : -1, OpMax(), -1, l);
    const int rr = base + TILE - 1 - i;
    const int nl = block_scan(rr < R && length(rr) >= m ? rr : BIG, OpMin(), BIG, l);
    const int nf = block_scan(rr + 1 < R && run_first[rr + 1] ? rr + 1 : BIG, OpMin(), BIG, l);
    xch[0][TILE - 1 - i] = nl;
    xch[1][TILE - 1 - i] = nf;
    __syncthreads();
    o.nl = xch[0][i];
    o.nf = xch[1][i];
    return o;
}

__global__ __launch_bounds__(TILE) void turns_runs_reduce_kernel(const int32_t* __restrict__ run_start, const uint8_t* __restrict__ run_first,
                                                                const int32_t* __restrict__ ctl, int N, int m, int32_t* __restrict__ agg,
                                                                const int32_t* status) {
    __shared__ ScanLds l;
    __shared__ int xch[2][TILE];
    if (*status) return;
    const int R = ctl[0], base = blockIdx.x * TILE;
    if (base >= R) return;
    const RunScan sc = run_scans(base, R, N, m, run_start, run_first, l, xch);
    int* g = agg + (int64_t)blockIdx.x * 4;
    if (threadIdx.x == TILE - 1) { g[0] = sc.pl; g[1] = sc.pf; }
    if (threadIdx.x == 0) { g[2] = sc.nl; g[3] = sc.nf; }
}

// component `comp` of agg [n, 4] -> its exclusive scan in place, forward or (mirror) from the end
template <class Op>
__device__ __forceinline__ void scan_component(int32_t* agg, int n, int comp, bool mirror, Op op, int ident, ScanLds& l) {
    int carry = ident;
    for (int c0 = 0; c0 < n; c0 += TILE) {
        const int k = c0 + (int)threadIdx.x, idx = mirror ? n - 1 - k : k;
        int tot;
        const int ex = block_scan_excl(k < n ? agg[(int64_t)idx * 4 + comp] : ident, op, ident, l, tot);
        if (k < n) agg[(int64_t)idx * 4 + comp] = op(carry, ex);
        carry = op(carry, tot);
    }
}

__global__ __launch_bounds__(TILE) void turns_agg_scan_kernel(int32_t* agg, const int32_t* __restrict__ ctl, const int32_t* status) {
    __shared__ ScanLds l;
    if (*status) return;
    const int R = ctl[0], n = (R + TILE - 1) / TILE;
    scan_component(agg, n, 0, false, OpMax(), -1, l);
    scan_component(agg, n, 1, false, OpMax(), -1, l);
    scan_component(agg, n, 2, true, OpMin(), BIG, l);
    scan_component(agg, n, 3, true, OpMin(), BIG, l);
}

__global__ __launch_bounds__(TILE) void turns_relabel_kernel(const int32_t* __restrict__ run_start, const uint8_t* __restrict__ run_first,
                                                            const int32_t* __restrict__ run_label, const int32_t* __restrict__ ctl, int N,
                                                            int m, const int32_t* __restrict__ agg, int32_t* __restrict__ new_label,
                                                            const int32_t* status) {
    __shared__ ScanLds l;
    __shared__ int xch[2][TILE];
    if (*status) return;
    const int R = ctl[0], base = blockIdx.x * TILE;
    if (base >= R) return;
    const RunScan sc = run_scans(base, R, N, m, run_start, run_first, l, xch);
    const int r = base + threadIdx.x;
    if (r >= R) return;
    const int* g = agg + (int64_t)blockIdx.x * 4;
    const int pl = OpMax()(sc.pl, g[0]), pf = OpMax()(sc.pf, g[1]), nl = OpMin()(sc.nl, g[2]), nf = OpMin()(sc.nf, g[3]);
    int src = r;
    if (sc.len < m) {
        if (pl >= 0 && pl >= pf) src = pl;
        else if (nl != BIG && nl < nf) src = nl;
    }
    new_label[r] = run_label[src];
}

__device__ __forceinline__ bool turn_head(int r, int R, const uint8_t* __restrict__ run_first, const int32_t* __restrict__ new_label) {
    return r < R && (run_first[r] || new_label[r] != new_label[r - 1]);      // (run 0 is the first of its item)
}

__global__ __launch_bounds__(TILE) void turns_count_kernel(const uint8_t* __restrict__ run_first, const int32_t* __restrict__ new_label,
                                                          const int32_t* __restrict__ ctl, int32_t* __restrict__ count,
                                                          const int32_t* status) {
    __shared__ int heads;
    if (*status) return;
    const int n = block_count(turn_head(blockIdx.x * TILE + threadIdx.x, ctl[0], run_first, new_label), &heads);
    if (threadIdx.x == 0) count[blockIdx.x] = n;
}

__global__ __launch_bounds__(TILE) void turns_scatter_kernel(const uint8_t* __restrict__ run_first, const int32_t* __restrict__ new_label,
                                                            const int32_t* __restrict__ run_start, const int32_t* __restrict__ ctl,
                                                            const int32_t* __restrict__ count, int32_t* __restrict__ turn_start,
                                                            int32_t* __restrict__ label, const int32_t* status) {
    __shared__ ScanLds l;
    if (*status) return;
    const int R = ctl[0], r = blockIdx.x * TILE + threadIdx.x;
    if (blockIdx.x * TILE >= R) return;
    const bool h = turn_head(r, R, run_first, new_label);
    const int inc = block_scan(h ? 1 : 0, OpSum(), 0, l);
    if (h) {
        const int k = count[blockIdx.x] + inc - 1;
        turn_start[k] = run_start[r];
        label[k] = new_label[r];
    }
}

__global__ __launch_bounds__(TILE) void turns_finish_kernel(const int32_t* __restrict__ turn_start, const int32_t* __restrict__ ctl,
                                                           const int64_t* __restrict__ off, int B, int N, int32_t* __restrict__ start,
                                                           int32_t* __restrict__ end, int32_t* __restrict__ purity,
                                                           int64_t* __restrict__ turn_ranges, int64_t* __restrict__ turn_offsets,
                                                           const int32_t* status) {
    if (*status) return;
    const int K = ctl[1];
    const int64_t k = (int64_t)blockIdx.x * TILE + threadIdx.x;
    if (k < K) {
        const int st = turn_start[k], en = k + 1 < K ? turn_start[k + 1] : N;
        const int lo = (int)off[item_of(off, B, st)];
        start[k] = st - lo;
        end[k] = en - lo;
        purity[k] = 0;
        if (turn_ranges) {
            turn_ranges[2 * k] = st;
            turn_ranges[2 * k + 1] = en;
        }
    }
    if (k <= B) {
        const int64_t f = off[k];
        turn_offsets[k] = f >= N ? K : last_le(turn_start, K, (int)f);
    }
}

__global__ __launch_bounds__(TILE) void turns_frames_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ turn_start,
                                                           const int32_t* __restrict__ label, const int32_t* __restrict__ ctl, int N,
                                                           int32_t* __restrict__ frame_labels, int32_t* purity, const int32_t* status) {
    __shared__ int bins[TILE];
    __shared__ int k0s;
    if (*status) return;
    const int K = ctl[1], i = threadIdx.x, t = blockIdx.x * TILE + i;
    bins[i] = 0;
    int k = 0, match = 0;
    if (t < N) {
        k = last_le(turn_start, K, t);
        const int lab = label[k];
        if (frame_labels) frame_labels[t] = lab;
        match = ids[t] == lab;
    }
    if (i == 0) k0s = k;
    __syncthreads();
    const int k0 = k0s;      // (a turn has a frame or more: the turns of a tile are k0 .. k0 + 255 at most)
    if (match) atomicAdd(&bins[k - k0], 1);
    __syncthreads();
    if (bins[i]) atomicAdd(&purity[k0 + i], bins[i]);
}

// ---------------------------------------------------------------- segment mean
__device__ __forceinline__ bool range_ok(int64_t a, int64_t b, int64_t N) { return a >= 0 && a <= b && b <= N; }

__global__ __launch_bounds__(TILE) void segmean_count_kernel(const int64_t* __restrict__ ranges, int G, int64_t N, int32_t* __restrict__ units,
                                                            int32_t* __restrict__ tile_sum, int32_t* status) {
    __shared__ ScanLds l;
    const int g = blockIdx.x * TILE + threadIdx.x;
    int u = 0;
    if (g < G) {
        const int64_t a = ranges[2 * (int64_t)g], b = ranges[2 * (int64_t)g + 1];
        if (range_ok(a, b, N)) {
            const int64_t c = segmean_chunks(a, b);
            u = c > BIG ? BIG : (int)c;
        } else {
            atomicOr(status, TAL_SEGMENT_MEAN_STATUS_BAD_RANGE);
        }
        units[g] = u;
    }
    const int inc = block_scan(u, OpSum(), 0, l);
    if (threadIdx.x == TILE - 1) tile_sum[blockIdx.x] = inc;
}

// units[g]: chunks of range g -> index of its first chunk
__global__ __launch_bounds__(TILE) void segmean_base_kernel(int32_t* __restrict__ units, int G, const int32_t* __restrict__ tile_sum) {
    __shared__ ScanLds l;
    const int g = blockIdx.x * TILE + threadIdx.x;
    int tot;
    const int ex = block_scan_excl(g < G ? units[g] : 0, OpSum(), 0, l, tot);
    if (g < G) units[g] = OpSum()(tile_sum[blockIdx.x], ex);
}

__global__ __launch_bounds__(TILE) void segmean_partial_kernel(const float* __restrict__ feat, int E, const int64_t* __restrict__ ranges, int G,
                                                              const int32_t* __restrict__ first, const int32_t* __restrict__ ctl,
                                                              int max_units, float* __restrict__ partial, int32_t* status) {
    __shared__ f32x4 slot[TILE];
    const int total = ctl[0];
    if (total > max_units) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, TAL_SEGMENT_MEAN_STATUS_TOO_MANY_CHUNKS);
        return;
    }
    if (*status & TAL_SEGMENT_MEAN_STATUS_BAD_RANGE) return;
    const int CT = E >> 2, RS = TILE / CT, q = threadIdx.x % CT, j = threadIdx.x / CT;
    for (int u = blockIdx.x; u < total; u += gridDim.x) {
        const int g = last_le(first, G, u);
        const int64_t a = ranges[2 * (int64_t)g], b = ranges[2 * (int64_t)g + 1];
        const int64_t r0 = a + (int64_t)(u - first[g]) * SEGMEAN_CHUNK, r1 = r0 + SEGMEAN_CHUNK < b ? r0 + SEGMEAN_CHUNK : b;
        if (j < RS) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int64_t row = r0 + j; row < r1; row += RS) acc += *reinterpret_cast<const f32x4*>(feat + row * E + 4 * q);
            slot[j * CT + q] = acc;
        }
        __syncthreads();
        if (j == 0) {
            f32x4 acc = slot[q];
            for (int jj = 1; jj < RS; ++jj) acc += slot[jj * CT + q];
            *reinterpret_cast<f32x4*>(partial + (int64_t)u * E + 4 * q) = acc;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void segmean_final_kernel(const float* __restrict__ partial, int E, const int64_t* __restrict__ ranges,
                                                          const int32_t* __restrict__ first, const int32_t* __restrict__ ctl, int max_units,
                                                          float* __restrict__ out, const int32_t* status) {
    if (ctl[0] > max_units || (*status & TAL_SEGMENT_MEAN_STATUS_BAD_RANGE)) return;
    const int g = blockIdx.x, q = blockIdx.y * 64 + threadIdx.x;
    if (q >= (E >> 2)) return;
    const int64_t a = ranges[2 * (int64_t)g], b = ranges[2 * (int64_t)g + 1];
    const int nc = (int)segmean_chunks(a, b);
    const float* p = partial + (int64_t)first[g] * E + 4 * q;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < nc; ++c) acc += *reinterpret_cast<const f32x4*>(p + (int64_t)c * E);
    if (nc > 0) {
        const float n = (float)(b - a);
        acc.x /= n; acc.y /= n; acc.z /= n; acc.w /= n;
    }
    *reinterpret_cast<f32x4*>(out + (int64_t)g * E + 4 * q) = acc;
}

}  // namespace

}  // namespace tal

using namespace tal;

extern "C" void tal_speaker_turns_tile(int* tile, int* max_half) {
    if (tile) *tile = TILE;
    if (max_half) *max_half = MAXW;
}

extern "C" size_t tal_speaker_turns_workspace_bytes(int64_t N) {
    if (N < 0 || N > TURNS_MAX_FRAMES) return 0;
    return (size_t)turns_layout(N).end;
}

extern "C" int tal_speaker_turns_fwd(const int32_t* ids, const int64_t* offsets_host, const int64_t* offsets_dev, int B, int num_ids,
                                     int smooth, int min_frames, int32_t* start, int32_t* end, int32_t* label, int32_t* purity,
                                     int32_t* frame_labels, int64_t* turn_ranges, int64_t* turn_offsets, int32_t* status, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    TAL_CHECK_ARG(B >= 0 && offsets_host && offsets_dev && turn_offsets && status, "tal_speaker_turns_fwd: null pointer or B=%d < 0", B);
    TAL_CHECK_ARG(num_ids > 0, "tal_speaker_turns_fwd: num_ids=%d", num_ids);
    TAL_CHECK_ARG(smooth >= 0 && smooth <= MAXW, "tal_speaker_turns_fwd: smooth=%d outside [0, TAL_TURNS_MAX_HALF = %d]", smooth, MAXW);
    TAL_CHECK_ARG(min_frames >= 1, "tal_speaker_turns_fwd: min_frames=%d < 1", min_frames);
    int64_t N64 = 0;
    TAL_CHECK_ARG(turns_offsets_ok(offsets_host, B, &N64), "tal_speaker_turns_fwd: offsets must start at 0 and ascend, at most %lld frames",
                  (long long)TURNS_MAX_FRAMES);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess) {
        set_error("tal_speaker_turns_fwd: cannot clear the status word");
        return TAL_EHIP;
    }
    if (N64 == 0) {
        if (hipMemsetAsync(turn_offsets, 0, ((size_t)B + 1) * sizeof(int64_t), s) != hipSuccess) {
            set_error("tal_speaker_turns_fwd: cannot clear turn_offsets");
            return TAL_EHIP;
        }
        return TAL_OK;
    }
    TAL_CHECK_ARG(ids && start && end && label && purity, "tal_speaker_turns_fwd: null pointer");
    const TurnsLayout L = turns_layout(N64);
    if (!workspace || workspace_bytes < (size_t)L.end) {
        set_error("tal_speaker_turns_fwd: workspace %zu < %zu bytes", workspace ? workspace_bytes : (size_t)0, (size_t)L.end);
        return TAL_ENOMEM;
    }
    TAL_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "tal_speaker_turns_fwd: the workspace must be 16-byte aligned");
    const int N = (int)N64, nt = (int)turns_tiles(N64);
    char* w = reinterpret_cast<char*>(workspace);
    int32_t* sm = reinterpret_cast<int32_t*>(w + L.smooth);
    uint8_t* fl = reinterpret_cast<uint8_t*>(w + L.flags);
    int32_t* rs = reinterpret_cast<int32_t*>(w + L.run_start);
    int32_t* rl = reinterpret_cast<int32_t*>(w + L.run_label);
    uint8_t* rf = reinterpret_cast<uint8_t*>(w + L.run_first);
    int32_t* nl = reinterpret_cast<int32_t*>(w + L.new_label);
    int32_t* ts = reinterpret_cast<int32_t*>(w + L.turn_start);
    int32_t* ca = reinterpret_cast<int32_t*>(w + L.count_a);
    int32_t* cb = reinterpret_cast<int32_t*>(w + L.count_b);
    int32_t* agg = reinterpret_cast<int32_t*>(w + L.agg);
    int32_t* ctl = reinterpret_cast<int32_t*>(w + L.ctl);
    ProfScope prof(PROF_OTHER, (double)N64 * 8, s);
    const dim3 grid((unsigned)nt), blk(TILE);
    hipLaunchKernelGGL(turns_mode_kernel, grid, blk, 0, s, ids, offsets_dev, B, N, num_ids, smooth, sm, fl, ca, status);
    hipLaunchKernelGGL(turns_scan_sum_kernel, dim3(1), blk, 0, s, ca, nt, ctl, status);
    hipLaunchKernelGGL(turns_runs_scatter_kernel, grid, blk, 0, s, sm, fl, ca, N, rs, rl, rf, status);
    hipLaunchKernelGGL(turns_runs_reduce_kernel, grid, blk, 0, s, rs, rf, ctl, N, min_frames, agg, status);
    hipLaunchKernelGGL(turns_agg_scan_kernel, dim3(1), blk, 0, s, agg, ctl, status);
    hipLaunchKernelGGL(turns_relabel_kernel, grid, blk, 0, s, rs, rf, rl, ctl, N, min_frames, agg, nl, status);
    hipLaunchKernelGGL(turns_count_kernel, grid, blk, 0, s, rf, nl, ctl, cb, status);
    hipLaunchKernelGGL(turns_scan_sum_kernel, dim3(1), blk, 0, s, cb, nt, ctl + 1, status);
    hipLaunchKernelGGL(turns_scatter_kernel, grid, blk, 0, s, rf, nl, rs, ctl, cb, ts, label, status);
    const int64_t fin = N64 > (int64_t)B + 1 ? N64 : (int64_t)B + 1;
    hipLaunchKernelGGL(turns_finish_kernel, dim3((unsigned)turns_tiles(fin)), blk, 0, s, ts, ctl, offsets_dev, B, N, start, end, purity,
                       turn_ranges, turn_offsets, status);
    hipLaunchKernelGGL(turns_frames_kernel, grid, blk, 0, s, ids, ts, label, ctl, N, frame_labels, purity, status);
    TAL_CHECK_LAUNCH("tal_speaker_turns_fwd");
    return TAL_OK;
}

extern "C" size_t tal_segment_mean_workspace_bytes(int64_t G, int64_t max_rows, int E) {
    if (!segmean_shape_ok(G, max_rows, E)) return 0;
    return (size_t)segmean_layout(G, max_rows, E).end;
}

extern "C" int tal_segment_mean_fwd(const float* feat, int64_t N, int E, const int64_t* ranges, int64_t G, int64_t max_rows, float* out,
                                    int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    TAL_CHECK_ARG(N >= 0 && segmean_shape_ok(G, max_rows, E),
                  "tal_segment_mean_fwd: N=%lld, G=%lld, max_rows=%lld must not be negative, E=%d a multiple of 4 in [4, %d]", (long long)N,
                  (long long)G, (long long)max_rows, E, SEGMEAN_MAX_E);
    TAL_CHECK_ARG(status, "tal_segment_mean_fwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess) {
        set_error("tal_segment_mean_fwd: cannot clear the status word");
        return TAL_EHIP;
    }
    if (G == 0) return TAL_OK;
    TAL_CHECK_ARG(ranges && out && (feat || N == 0), "tal_segment_mean_fwd: null pointer");
    TAL_CHECK_ARG(((reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
                  "tal_segment_mean_fwd: feat and out must be 16-byte aligned");
    const SegmeanLayout L = segmean_layout(G, max_rows, E);
    if (!workspace || workspace_bytes < (size_t)L.end) {
        set_error("tal_segment_mean_fwd: workspace %zu < %zu bytes", workspace ? workspace_bytes : (size_t)0, (size_t)L.end);
        return TAL_ENOMEM;
    }
    TAL_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "tal_segment_mean_fwd: the workspace must be 16-byte aligned");
    char* w = reinterpret_cast<char*>(workspace);
    int32_t* units = reinterpret_cast<int32_t*>(w + L.units);
    int32_t* tsum = reinterpret_cast<int32_t*>(w + L.tile_sum);
    int32_t* ctl = reinterpret_cast<int32_t*>(w + L.ctl);
    float* partial = reinterpret_cast<float*>(w + L.partial);
    const int ntg = (int)turns_tiles(G), max_units = (int)segmean_max_units(G, max_rows);
    const int64_t wgs = (int64_t)8 * device_cus();
    ProfScope prof(PROF_OTHER, (double)max_rows * E * 4, s);
    hipLaunchKernelGGL(segmean_count_kernel, dim3((unsigned)ntg), dim3(TILE), 0, s, ranges, (int)G, N, units, tsum, status);
    hipLaunchKernelGGL(turns_scan_sum_kernel, dim3(1), dim3(TILE), 0, s, tsum, ntg, ctl, (const int32_t*)nullptr);
    hipLaunchKernelGGL(segmean_base_kernel, dim3((unsigned)ntg), dim3(TILE), 0, s, units, (int)G, tsum);
    hipLaunchKernelGGL(segmean_partial_kernel, dim3((unsigned)(max_units < wgs ? max_units : wgs)), dim3(TILE), 0, s, feat, E, ranges,
                       (int)G, units, ctl, max_units, partial, status);
    hipLaunchKernelGGL(segmean_final_kernel, dim3((unsigned)G, (unsigned)((E / 4 + 63) / 64)), dim3(64), 0, s, partial, E, ranges, units, ctl,
                       max_units, out, status);
    TAL_CHECK_LAUNCH("tal_segment_mean_fwd");
    return TAL_OK;
}
