// WER / WDER scoring on the device: unit-cost Levenshtein distance and the alignment of wder.align_opcodes for a batch of ragged
// pairs of int32 id sequences (equal words = equal ids).  Integers only; every result is exact.
//
// TWO TABLES, ONE SWEEP.  D is the Levenshtein table (D[i][0] = i, D[0][j] = j, D[i][j] = min(D[i-1][j-1] + (a != b), D[i-1][j] + 1,
// D[i][j-1] + 1)); M is the match-count table of align_opcodes (M[i][0] = M[0][j] = 0; sm = M[i-1][j-1] + eq, im = M[i][j-1],
// dm = M[i-1][j]; M[i][j] = max) with the back-pointer 0 (diagonal) if sm == max, else 1 (insert) if im == max, else 2 (delete).
//
// TILES.  The tables are cut into tiles of ER = 64 rows x EC = 128 columns (TAL_EDIT_TILE_*; profiles/edit_align.txt has the widths
// tried); one wave sweeps a tile.  The sweep is skewed: lane r owns
// row r of the tile and handles column s - r at step s, so the cell above it was finished by lane r - 1 one step before and comes
// over by a one-lane DPP shift (wave_shr:1; no LDS).  The same shift hands the b ids down the lanes: lane 0 picks id s out of a
// 64-column chunk register (v_readlane), every other lane takes its neighbour's.  D, M and the diagonal values stay in registers.
//   Boundaries travel through the workspace: a tile reads the row above it (D and M, 64 columns per coalesced load, one chunk ahead),
//   the column to its left (one coalesced load), and the corner; it writes its bottom row (lane 63's values gathered into a chunk
//   register lane by lane and stored 64 columns at a time), its right column (one coalesced store) and the next corner.  Every row
//   segment belongs to a tile column and every column segment to a tile row, and the tiles of one launch have distinct tile rows and
//   columns: no two workgroups of a launch touch the same word.
//   Back-pointers: 2 bits per cell (0 diagonal / replace, 1 insert, 2 delete, 3 diagonal / equal -- the traceback needs no ids),
//   ER * EC / 4 bytes per tile.  Lane r packs the codes of 16 consecutive steps into a word; all 64 lanes store their word together (256 bytes,
//   coalesced).  Step s of lane r goes to slot s mod EC -- a lane's EC steps [r, r + EC) hit every slot once, so the skew costs no
//   memory: word (slot / 16) * 64 + r, bits 2 (slot % 16).  The one word of a lane that the wrap cuts in two is completed from a
//   register (`firstw`) when its second half arrives.  All table offsets are 64-bit.
//
// BETWEEN TILES.  Launch d covers every tile (ti, tj) with ti + tj = d of every pair; dependencies are carried by stream order only
// (no flags, no spins).  Launches per call = the largest number of tile anti-diagonals of any pair, + 1 for the finish kernel.
//
// FINISH (one workgroup per pair): walks the back-pointers from (m, n) to (0, 0) out of LDS-staged tiles (boundary rule: i == 0 ->
// insert, j == 0 -> delete), buffers 1024 steps in LDS, and per buffer-full writes the tags (coalesced) into a scratch line and adds
// the (ref label, hyp label) cell of every equal / replace step with LDS atomics (global atomics beyond 4096 cells).  The scratch
// line is then copied in forward order.
#include "common.h"

namespace tal {

namespace {

constexpr int ER = TAL_EDIT_TILE_ROWS, EC = TAL_EDIT_TILE_COLS;
static_assert(ER == 64, "one lane per tile row");
static_assert(EC % 64 == 0 && EC >= 64 && (EC & (EC - 1)) == 0, "the slot wrap needs a power of two that holds whole chunks");
constexpr int TILE_WORDS = ER * EC / 16;
constexpr int WALK_BUF = 1024;
constexpr int LDS_CELLS = 4096;      // label cells counted in LDS
constexpr int DESC_WORDS = 8;        // int64 per pair: a_off, m, b_off, n, ws_off, path_off, -, -

struct Layout {      // byte offsets inside a pair's workspace region (all multiples of 16)
    int64_t rowD, rowM, colD, colM, cornD, cornM, line, table, end;
};

__host__ __device__ inline int64_t up16(int64_t x) { return (x + 15) & ~(int64_t)15; }

__host__ __device__ inline Layout pair_layout(int64_t m, int64_t n, bool want_path) {
    // (a pair with an empty side has no tiles, rows or columns: only the scratch line of its one-sided path)
    const int64_t nti = n > 0 ? (m + ER - 1) / ER : 0, ntj = m > 0 ? (n + EC - 1) / EC : 0;
    Layout l;
    int64_t o = 0;
    l.rowD = o; o += ntj * EC * 4;
    l.rowM = o; if (want_path) o += ntj * EC * 4;
    l.colD = o; o += nti * ER * 4;
    l.colM = o; if (want_path) o += nti * ER * 4;
    l.cornD = o; o += up16(ntj * 4);
    l.cornM = o; if (want_path) o += up16(ntj * 4);
    l.line = o; if (want_path) o += up16(m + n);
    l.table = o; if (want_path) o += nti * ntj * (int64_t)TILE_WORDS * 4;
    l.end = o;
    return l;
}

// lane l takes lane l - 1's `v`; lane 0 takes `first`
__device__ __forceinline__ int shr1(int v, int first) { return __builtin_amdgcn_update_dpp(first, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }

template <bool PATH>
__global__ __launch_bounds__(64) void edit_sweep_kernel(const int64_t* __restrict__ desc, const int32_t* __restrict__ a_all,
                                                        const int32_t* __restrict__ b_all, char* ws, int d, int64_t* stats) {
    const int p = blockIdx.y;
    const int64_t* dp = desc + (int64_t)p * DESC_WORDS;
    const int64_t m = dp[1], n = dp[3];
    if (m == 0 || n == 0) return;
    const int64_t nti = (m + ER - 1) / ER, ntj = (n + EC - 1) / EC;
    const int64_t lo = d - (ntj - 1) > 0 ? d - (ntj - 1) : 0, hi = nti - 1 < d ? nti - 1 : d;
    const int64_t ti = lo + blockIdx.x;
    if (ti > hi) return;
    const int64_t tj = d - ti;
    const int lane = threadIdx.x;
    const int64_t i0 = ti * ER, j0 = tj * EC;
    const int rh = (int)(m - i0 < ER ? m - i0 : ER), cw = (int)(n - j0 < EC ? n - j0 : EC);
    const bool has_below = ti + 1 < nti, has_right = tj + 1 < ntj;
    const Layout L = pair_layout(m, n, PATH);
    char* base = ws + dp[4];
    int* rowD = reinterpret_cast<int*>(base + L.rowD) + j0;
    int* rowM = reinterpret_cast<int*>(base + L.rowM) + j0;
    int* colD = reinterpret_cast<int*>(base + L.colD) + i0;
    int* colM = reinterpret_cast<int*>(base + L.colM) + i0;
    int* cornD = reinterpret_cast<int*>(base + L.cornD) + tj;
    int* cornM = reinterpret_cast<int*>(base + L.cornM) + tj;
    unsigned* tile = reinterpret_cast<unsigned*>(base + L.table) + (ti * ntj + tj) * (int64_t)TILE_WORDS;
    const int32_t* a = a_all + dp[0] + i0;
    const int32_t* b = b_all + dp[2] + j0;

    const int av = lane < rh ? a[lane] : 0;
    // left column D[i0 + 1 + lane][j0] (and M): computed on the table's edge, else the right column of the tile to the left
    const int leftD = tj == 0 ? (int)i0 + lane + 1 : colD[lane];
    int leftM = 0, cornerM = 0;
    if (PATH && tj != 0) leftM = colM[lane];
    const int cornerD = ti == 0 ? (int)j0 : (tj == 0 ? (int)i0 : cornD[0]);
    if (PATH && ti != 0 && tj != 0) cornerM = cornM[0];
    int curD = leftD, curM = leftM;
    int diagD = shr1(leftD, cornerD), diagM = PATH ? shr1(leftM, cornerM) : 0;
    int bv = 0;
    unsigned w = 0, firstw = 0;
    int outD = 0, outM = 0;

    // chunk c of the row above: lane l holds column 64 c + l (D[i0][j0 + 1 + col], M, and b[j0 + col])
    auto load_chunk = [&](int c, int& tD, int& tM, int& tb) {
        const int col = 64 * c + lane;
        tD = (int)j0 + col + 1;
        tM = 0;
        tb = 0;
        if (col < cw) {
            tb = b[col];
            if (ti != 0) {
                tD = rowD[col];
                if (PATH) tM = rowM[col];
            }
        }
    };
    const int nsteps = (cw + ER - 1 + 15) & ~15;      // lane 63 finishes column cw - 1 at step cw + 62; whole 16-step groups
    const int nchunks = (nsteps + 63) / 64;
    int nD, nM, nb;
    load_chunk(0, nD, nM, nb);
    for (int c = 0; c < nchunks; ++c) {
        const int topD = nD, topM = nM, topb = nb;
        if (64 * (c + 1) < cw) load_chunk(c + 1, nD, nM, nb);      // one chunk ahead
        const int gend = nsteps - 64 * c < 64 ? (nsteps - 64 * c) / 16 : 4;
        for (int q = 0; q < gend; ++q) {
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int sl = 16 * q + t, s = 64 * c + sl;
                const int tD = __builtin_amdgcn_readlane(topD, sl), tb = __builtin_amdgcn_readlane(topb, sl);
                const int upD = shr1(curD, tD);
                bv = shr1(bv, tb);
                int upM = 0;
                if (PATH) upM = shr1(curM, __builtin_amdgcn_readlane(topM, sl));
                const int jl = s - lane;
                const bool active = jl >= 0 && jl < cw;
                const int eq = av == bv ? 1 : 0;
                const int dd = diagD + 1 - eq, ud = (upD < curD ? upD : curD) + 1;
                const int newD = dd < ud ? dd : ud;
                if (PATH) {
                    const int sm = diagM + eq, im = curM, dm = upM;
                    int mx = sm > im ? sm : im;
                    mx = dm > mx ? dm : mx;
                    const unsigned code = sm == mx ? (eq ? 3u : 0u) : (im == mx ? 1u : 2u);
                    w |= active ? code << (2 * t) : 0u;
                    diagM = active ? upM : diagM;
                    curM = active ? mx : curM;
                }
                diagD = active ? upD : diagD;
                curD = active ? newD : curD;
                if (has_below) {
                    // lane 63 (the tile's bottom row) has just finished column s - 63: lane (column % 64) keeps it
                    const int j63 = s - 63;
                    if (j63 >= 0 && j63 < cw) {
                        const int vD = __builtin_amdgcn_readlane(curD, 63);
                        const bool mine = lane == (j63 & 63);
                        outD = mine ? vD : outD;
                        if (PATH) {
                            const int vM = __builtin_amdgcn_readlane(curM, 63);
                            outM = mine ? vM : outM;
                        }
                        if ((j63 & 63) == 63 || j63 == cw - 1) {
                            if (lane <= (j63 & 63)) {
                                rowD[(j63 & ~63) + lane] = outD;
                                if (PATH) rowM[(j63 & ~63) + lane] = outM;
                            }
                        }
                    }
                }
            }
            if (PATH) {
                // the 16 codes of this group: slot group g = (s / 16) mod (EC / 16); a lane's first group (the one that holds step
                // `lane`) is cut by the wrap and completed when the group EC / 16 later arrives
                const int g = 4 * c + q, rq = lane >> 4;
                if (g == rq) firstw = w;
                if (g < EC / 16) {
                    tile[g * 64 + lane] = w;
                } else {
                    const int gg = g - EC / 16;
                    if (rq == gg)
                        tile[gg * 64 + lane] = w | firstw;
                    else if (rq > gg)
                        tile[gg * 64 + lane] = w;
                }
                w = 0;
            }
        }
    }
    if (has_right) {
        colD[lane] = curD;
        if (PATH) colM[lane] = curM;
    }
    if (has_below && lane == ER - 1) {
        cornD[0] = leftD;
        if (PATH) cornM[0] = leftM;
    }
    if (!has_below && !has_right && lane == rh - 1) stats[(int64_t)p * 4] = curD;
}

// one workgroup per pair: distance of an empty pair, traceback, label counts
__global__ __launch_bounds__(256) void edit_finish_kernel(const int64_t* __restrict__ desc, const char* ws, int want_path,
                                                          const int32_t* __restrict__ a_lab, const int32_t* __restrict__ b_lab, int Ka,
                                                          int Kb, int64_t* stats, uint8_t* path, int64_t* counts) {
    __shared__ unsigned tile[TILE_WORDS];
    __shared__ uint8_t tagbuf[WALK_BUF];
    __shared__ int ibuf[WALK_BUF], jbuf[WALK_BUF];
    __shared__ unsigned lcnt[LDS_CELLS];
    __shared__ unsigned tally[2];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int64_t* dp = desc + (int64_t)p * DESC_WORDS;
    const int64_t m = dp[1], n = dp[3];
    int64_t* st = stats + (int64_t)p * 4;
    if ((m == 0 || n == 0) && tid == 0) st[0] = m > n ? m : n;
    if (!want_path) {
        if (tid == 0) st[1] = st[2] = st[3] = 0;
        return;
    }
    const bool labels = counts != nullptr;
    const int cells = labels ? Ka * Kb : 0;
    const bool lds_counts = cells <= LDS_CELLS;
    int64_t* cnt = labels ? counts + (int64_t)p * cells : nullptr;
    if (lds_counts) {
        for (int i = tid; i < cells; i += 256) lcnt[i] = 0;
    } else {
        for (int i = tid; i < cells; i += 256) cnt[i] = 0;
        __threadfence();
    }
    if (tid < 2) tally[tid] = 0;
    __syncthreads();

    const int64_t ntj = (n + EC - 1) / EC;
    const Layout L = pair_layout(m, n, true);
    const char* base = ws + dp[4];
    const unsigned* table = reinterpret_cast<const unsigned*>(base + L.table);
    uint8_t* line = reinterpret_cast<uint8_t*>(const_cast<char*>(base) + L.line);
    const int32_t* la = labels ? a_lab + dp[0] : nullptr;
    const int32_t* lb = labels ? b_lab + dp[2] : nullptr;
    unsigned my_eq = 0, my_rep = 0;

    // `k` buffered steps go out: tags to the scratch line (walk order), label cells of the diagonal steps
    auto flush = [&](int64_t done, int k) {
        __syncthreads();
        for (int t = tid; t < k; t += 256) {
            const unsigned tag = tagbuf[t];
            line[done + t] = (uint8_t)tag;
            if (tag <= 1) {
                if (tag == 0) ++my_eq; else ++my_rep;
                if (labels) {
                    const int x = la[ibuf[t]], y = lb[jbuf[t]];
                    if (x >= 0 && x < Ka && y >= 0 && y < Kb) {
                        if (lds_counts)
                            atomicAdd(&lcnt[x * Kb + y], 1u);
                        else
                            atomicAdd(reinterpret_cast<unsigned long long*>(cnt) + (x * Kb + y), 1ull);
                    }
                }
            }
        }
        __syncthreads();
    };

    // every thread walks the same path (uniform control flow; the LDS reads are broadcasts)
    int64_t i = m, j = n, done = 0, cur_tile = -1;
    int k = 0;
    while (i > 0 || j > 0) {
        unsigned code;
        if (i == 0) {
            code = 1;
        } else if (j == 0) {
            code = 2;
        } else {
            const int64_t ti = (i - 1) / ER, tj = (j - 1) / EC, tidx = ti * ntj + tj;
            if (tidx != cur_tile) {
                __syncthreads();
                const uint4* src = reinterpret_cast<const uint4*>(table + tidx * (int64_t)TILE_WORDS);
                for (int q = tid; q < TILE_WORDS / 4; q += 256) reinterpret_cast<uint4*>(tile)[q] = src[q];
                __syncthreads();
                cur_tile = tidx;
            }
            const int r = (int)((i - 1) % ER), jl = (int)((j - 1) % EC), slot = (r + jl) & (EC - 1);
            code = (tile[(slot >> 4) * 64 + r] >> (2 * (slot & 15))) & 3u;
        }
        // path tags: 0 equal, 1 replace, 2 insert, 3 delete
        const unsigned tag = code == 3 ? 0u : (code == 0 ? 1u : (code == 1 ? 2u : 3u));
        if (tid == 0) {
            tagbuf[k] = (uint8_t)tag;
            ibuf[k] = (int)(i - 1);
            jbuf[k] = (int)(j - 1);
        }
        if (tag <= 1) { --i; --j; } else if (tag == 2) { --j; } else { --i; }
        if (++k == WALK_BUF) {
            flush(done, k);
            done += k;
            k = 0;
        }
    }
    flush(done, k);
    done += k;

    // forward order; the rest of the pair's m + n bytes is TAL_EDIT_TAG_NONE
    uint8_t* out = path + dp[5];
    for (int64_t t = tid; t < m + n; t += 256) out[t] = t < done ? line[done - 1 - t] : (uint8_t)TAL_EDIT_TAG_NONE;
    if (my_eq) atomicAdd(&tally[0], my_eq);
    if (my_rep) atomicAdd(&tally[1], my_rep);
    __syncthreads();
    if (tid == 0) {
        st[1] = done;
        st[2] = tally[0];
        st[3] = tally[1];
    }
    if (labels && lds_counts)
        for (int c = tid; c < cells; c += 256) cnt[c] = lcnt[c];
}

struct Plan {
    size_t ws_bytes;
    int64_t diagonals, max_tiles, path_bytes;
};

// host: offsets [P + 1] -> the descriptor table (may be NULL) and the call's geometry; false on a bad offset table
bool edit_plan(int P, const int64_t* a_off, const int64_t* b_off, bool want_path, int64_t* desc, Plan& pl) {
    int64_t ws = 0, path = 0;
    pl.diagonals = pl.max_tiles = 0;
    for (int p = 0; p < P; ++p) {
        const int64_t m = a_off[p + 1] - a_off[p], n = b_off[p + 1] - b_off[p];
        if (m < 0 || n < 0 || a_off[p] < 0 || b_off[p] < 0 || m > INT32_MAX - 2 * EC || n > INT32_MAX - 2 * EC) return false;
        if (desc) {
            int64_t* dp = desc + (int64_t)p * DESC_WORDS;
            dp[0] = a_off[p]; dp[1] = m; dp[2] = b_off[p]; dp[3] = n; dp[4] = ws; dp[5] = path; dp[6] = dp[7] = 0;
        }
        if (m > 0 && n > 0) {
            const int64_t nti = cdiv(m, ER), ntj = cdiv(n, EC), diag = nti + ntj - 1, across = nti < ntj ? nti : ntj;
            pl.diagonals = diag > pl.diagonals ? diag : pl.diagonals;
            pl.max_tiles = across > pl.max_tiles ? across : pl.max_tiles;
        }
        ws += pair_layout(m, n, want_path).end;
        path += m + n;
    }
    pl.ws_bytes = (size_t)ws;
    pl.path_bytes = path;
    return true;
}

}  // namespace

}  // namespace tal

using namespace tal;

extern "C" void tal_edit_align_tile(int* rows, int* cols) {
    if (rows) *rows = ER;
    if (cols) *cols = EC;
}

extern "C" size_t tal_edit_align_workspace_bytes(int P, const int64_t* a_off, const int64_t* b_off, int want_path) {
    Plan pl;
    if (P <= 0 || !a_off || !b_off || !edit_plan(P, a_off, b_off, want_path != 0, nullptr, pl)) return 0;
    return pl.ws_bytes;
}

extern "C" int tal_edit_align_plan(int P, const int64_t* a_off, const int64_t* b_off, int want_path, int64_t* desc, size_t* workspace_bytes,
                                   int64_t* path_bytes, int* launches) {
    TAL_CHECK_ARG(P >= 0 && P <= 65535, "tal_edit_align_plan: P=%d outside [0, 65535]", P);
    TAL_CHECK_ARG(P == 0 || (a_off && b_off && desc), "tal_edit_align_plan: null pointer");
    Plan pl;
    TAL_CHECK_ARG(edit_plan(P, a_off, b_off, want_path != 0, desc, pl), "tal_edit_align_plan: offsets must be non-negative and ascending, "
                  "a side at most 2^31 - 1 - %d ids", 2 * EC);
    if (workspace_bytes) *workspace_bytes = pl.ws_bytes;
    if (path_bytes) *path_bytes = pl.path_bytes;
    if (launches) *launches = P == 0 ? 0 : (int)pl.diagonals + 1;
    return TAL_OK;
}

extern "C" int tal_edit_align_fwd(const int64_t* desc_host, const int64_t* desc_dev, int P, const int32_t* a, const int32_t* b,
                                  const int32_t* a_lab, const int32_t* b_lab, int Ka, int Kb, int64_t* stats, uint8_t* path,
                                  int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    TAL_CHECK_ARG(P >= 0 && P <= 65535, "tal_edit_align_fwd: P=%d outside [0, 65535]", P);
    if (P == 0) return TAL_OK;
    TAL_CHECK_ARG(desc_host && desc_dev && stats, "tal_edit_align_fwd: null pointer");
    const bool want_path = path != nullptr;
    TAL_CHECK_ARG(!counts || (want_path && Ka > 0 && Kb > 0 && (int64_t)Ka * Kb <= (1 << 24)),
                  "tal_edit_align_fwd: counts need the path and 0 < Ka * Kb <= 2^24 (Ka=%d, Kb=%d)", Ka, Kb);
    // the descriptors are re-derived from their own (offset, length) columns: a table that tal_edit_align_plan did not write for this
    // `want_path` is refused, and the pair regions are known to lie inside the workspace before anything is launched
    int64_t ws = 0, po = 0, diagonals = 0, max_tiles = 0, ids_a = 0, ids_b = 0;
    for (int p = 0; p < P; ++p) {
        const int64_t* dp = desc_host + (int64_t)p * DESC_WORDS;
        const int64_t m = dp[1], n = dp[3];
        TAL_CHECK_ARG(m >= 0 && n >= 0 && dp[0] >= 0 && dp[2] >= 0 && m <= INT32_MAX - 2 * EC && n <= INT32_MAX - 2 * EC && dp[4] == ws && dp[5] == po,
                      "tal_edit_align_fwd: descriptor %d was not written by tal_edit_align_plan(want_path=%d)", p, (int)want_path);
        if (m > 0 && n > 0) {
            const int64_t nti = cdiv(m, ER), ntj = cdiv(n, EC), diag = nti + ntj - 1, across = nti < ntj ? nti : ntj;
            diagonals = diag > diagonals ? diag : diagonals;
            max_tiles = across > max_tiles ? across : max_tiles;
        }
        ws += pair_layout(m, n, want_path).end;
        po += m + n;
        ids_a += m;
        ids_b += n;
    }
    TAL_CHECK_ARG((ids_a == 0 || a) && (ids_b == 0 || b), "tal_edit_align_fwd: null pointer");
    TAL_CHECK_ARG(!counts || ((ids_a == 0 || a_lab) && (ids_b == 0 || b_lab)), "tal_edit_align_fwd: counts need both label arrays");
    if ((size_t)ws > 0 && (!workspace || workspace_bytes < (size_t)ws)) {
        set_error("tal_edit_align_fwd: workspace %zu < %zu bytes", workspace ? workspace_bytes : (size_t)0, (size_t)ws);
        return TAL_ENOMEM;
    }
    TAL_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "tal_edit_align_fwd: the workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    char* wsp = reinterpret_cast<char*>(workspace);
    if (diagonals > 0) {
        ProfScope prof(PROF_OTHER, (double)ws, s);
        const dim3 grid((unsigned)max_tiles, (unsigned)P);
        for (int64_t d = 0; d < diagonals; ++d) {
            if (want_path)
                hipLaunchKernelGGL(edit_sweep_kernel<true>, grid, dim3(64), 0, s, desc_dev, a, b, wsp, (int)d, stats);
            else
                hipLaunchKernelGGL(edit_sweep_kernel<false>, grid, dim3(64), 0, s, desc_dev, a, b, wsp, (int)d, stats);
        }
        TAL_CHECK_LAUNCH("edit_align(sweep)");
    }
    ProfScope prof(PROF_OTHER, (double)po, s);
    hipLaunchKernelGGL(edit_finish_kernel, dim3((unsigned)P), dim3(256), 0, s, desc_dev, wsp, (int)want_path, a_lab, b_lab, Ka, Kb, stats,
                       path, counts);
    TAL_CHECK_LAUNCH("edit_align(finish)");
    return TAL_OK;
}
