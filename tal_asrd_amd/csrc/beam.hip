// Beam-search candidate selection: System.generate, tal/asr/system.py:141-160.
//   total = logprobs + scores[row]; rows of finished beams -> -inf; per batch item flatten the
//   cur_beam x V candidates and take the top-k (values descending, lowest flat index first on ties).
// One workgroup per batch item; k (the beam width) is small, so the top-k is k rounds of a
// block-wide arg-max over the candidates that have not been taken yet.
//
// Device-resident search (tal_beam_ctx, System.generate(search="device")): the same selection straight from the raw
// logits, spread over chunks of the vocabulary, and the loop's bookkeeping (system.py:141-219) as device state -- see the
// second half of this file.
#include "common.h"

namespace tal {

constexpr int TOPK_MAX = 64;

__global__ __launch_bounds__(256) void beam_topk_kernel(const float* __restrict__ logprobs,
                                                       const float* __restrict__ row_score,
                                                       const uint8_t* __restrict__ row_done, int cur_beam, int V,
                                                       int k, float* __restrict__ out_val,
                                                       int64_t* __restrict__ out_idx) {
    __shared__ float s_val[4];
    __shared__ int64_t s_idx[4];
    __shared__ int64_t taken[TOPK_MAX];
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t n = (int64_t)cur_beam * V;
    const float* lp = logprobs + (int64_t)b * n;
    for (int j = 0; j < k; ++j) {
        float best = -INFINITY;
        int64_t bi = INT64_MAX;
        for (int64_t i = tid; i < n; i += 256) {
            const int r = (int)(i / V);
            const int row = b * cur_beam + r;
            float v = lp[i] + (row_score ? row_score[row] : 0.f);
            if (row_done && row_done[row]) v = -INFINITY;
            bool skip = false;
            for (int t = 0; t < j; ++t) skip |= (taken[t] == i);
            if (!skip && (v > best || (v == best && i < bi))) {
                best = v;
                bi = i;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(best, off, 64);
            const int64_t oi = __shfl_xor(bi, off, 64);
            if (ov > best || (ov == best && oi < bi)) {
                best = ov;
                bi = oi;
            }
        }
        if (lane == 0) {
            s_val[w] = best;
            s_idx[w] = bi;
        }
        __syncthreads();
        if (tid == 0) {
            for (int q = 1; q < 4; ++q)
                if (s_val[q] > best || (s_val[q] == best && s_idx[q] < bi)) {
                    best = s_val[q];
                    bi = s_idx[q];
                }
            // every candidate already taken or -inf everywhere: fall back to the lowest untaken index
            if (bi == INT64_MAX) {
                bi = 0;
                for (bool clash = true; clash;) {
                    clash = false;
                    for (int t = 0; t < j; ++t)
                        if (taken[t] == bi) {
                            ++bi;
                            clash = true;
                        }
                }
                best = -INFINITY;
            }
            taken[j] = bi;
            out_val[(int64_t)b * k + j] = best;
            out_idx[(int64_t)b * k + j] = bi;
        }
        __syncthreads();
    }
}

}  // namespace tal

using namespace tal;

extern "C" int tal_beam_topk(const float* logprobs, const float* row_score, const uint8_t* row_done, int B,
                             int cur_beam, int V, int k, float* out_val, int64_t* out_idx, void* stream) {
    TAL_CHECK_ARG(logprobs && out_val && out_idx, "tal_beam_topk: null pointer");
    TAL_CHECK_ARG(B > 0 && cur_beam > 0 && V > 0 && k > 0 && k <= TOPK_MAX && (int64_t)k <= (int64_t)cur_beam * V,
                  "tal_beam_topk: bad shape B=%d beams=%d V=%d k=%d", B, cur_beam, V, k);
    hipLaunchKernelGGL(beam_topk_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, logprobs, row_score,
                       row_done, cur_beam, V, k, out_val, out_idx);
    TAL_CHECK_LAUNCH("tal_beam_topk");
    return TAL_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Device-resident beam search: the per-step work of System.generate (tal/asr/system.py:124-219) after the logits.
//   select  = log_softmax + LM bias + score add + done mask + per-item top-beam, straight from the raw logits:
//             (1) one workgroup per (vocabulary chunk, row): the row's max / log-sum-exp in the order of
//                 log_softmax_row_block_kernel (every workgroup of a row recomputes them: 2 x V / 256 loads and expf per
//                 thread, from L2), then the chunk's best min(beam, chunk) candidates;
//             (2) one workgroup per item merges its cur_beam x chunks x beam partial candidates.
//             Candidates are ordered as beam_topk_kernel orders them: value descending, lowest flat index on ties, NaN
//             values last by index with -inf reported (its all-masked fallback).  That order is total and strict, so
//             round j simply takes the best candidate that is worse than round j - 1's: no list of taken indices.
//   advance = re-thread + append + scores + speaker rows + finish records + counters, one workgroup per row slot.
// No workgroup reads what another one writes in the same launch; the launches of a step hand over by stream order.
namespace tal {

constexpr int BEAM_ROWS_MAX = 512;      // above it tal_log_softmax_rows sums a row in another order
constexpr int BEAM_CHUNK = 2048;        // vocabulary entries per selection workgroup (at least 2, at most 64 chunks per row)

struct BeamLayout {
    size_t ctl, scores, done, rec_step, rec_score, rec_tokens, tok0, tok1, sel_val, sel_idx, state_end, part_val, part_idx,
        spk_hist, parent, total;
    int C, chunk;
};
static inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }
static inline int beam_chunks(int V) {
    const int64_t c = cdiv(V, BEAM_CHUNK);
    return V < 2 ? 1 : (int)(c < 2 ? 2 : (c > 64 ? 64 : c));
}
static bool beam_layout(int B, int beam, int L0, int length, int V, int ns, BeamLayout& l) {
    if (B <= 0 || beam <= 0 || beam > TOPK_MAX || L0 <= 0 || length <= 0 || V <= 0 || ns < 0 || (int64_t)B * beam > BEAM_ROWS_MAX ||
        (int64_t)L0 + length > 65535)      // (a grid dimension of the gather)
        return false;
    const size_t R = (size_t)B * beam, Lmax = (size_t)L0 + length;
    l.C = beam_chunks(V);
    l.chunk = (int)cdiv(V, l.C);
    size_t o = 0;
    l.ctl = o;        o = up16(o + 4 * sizeof(uint32_t));
    l.scores = o;     o = up16(o + R * sizeof(float));
    l.done = o;       o = up16(o + R);
    l.rec_step = o;   o = up16(o + R * sizeof(int32_t));
    l.rec_score = o;  o = up16(o + R * sizeof(float));
    l.rec_tokens = o; o = up16(o + R * Lmax * sizeof(int64_t));
    l.tok0 = o;       o = up16(o + R * Lmax * sizeof(int64_t));
    l.tok1 = o;       o = up16(o + R * Lmax * sizeof(int64_t));
    l.sel_val = o;    o = up16(o + R * sizeof(float));
    l.sel_idx = o;    o = up16(o + R * sizeof(int64_t));
    l.state_end = o;
    l.part_val = o;   o = up16(o + R * l.C * beam * sizeof(float));
    l.part_idx = o;   o = up16(o + R * l.C * beam * sizeof(int64_t));
    l.spk_hist = o;   o = up16(o + (size_t)length * R * ns * sizeof(float));
    l.parent = o;     o = up16(o + (ns > 0 ? (size_t)length * R * sizeof(int32_t) : 0));
    l.total = o;
    return true;
}

// is candidate 1 taken before candidate 2?  (beam_topk_kernel: v > best || (v == best && i < bi); a NaN never wins there and is
// handed out by its fallback, lowest index first, once nothing else is left)
__device__ __forceinline__ bool cand_before(float v1, int64_t i1, float v2, int64_t i2) {
    const bool n1 = v1 != v1, n2 = v2 != v2;
    if (n1 != n2) return n2;
    if (n1) return i1 < i2;
    return v1 > v2 || (v1 == v2 && i1 < i2);
}
#define BEAM_NONE_V __int_as_float(0x7fc00000)      // "no candidate": a NaN with the largest index comes after every real one
#define BEAM_NONE_I INT64_MAX

// the workgroup's first candidate in that order, in every thread
__device__ __forceinline__ void block_first(float& v, int64_t& i, float* s_val, int64_t* s_idx) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int64_t oi = __shfl_xor(i, off, 64);
        if (cand_before(ov, oi, v, i)) {
            v = ov;
            i = oi;
        }
    }
    if (lane == 0) {
        s_val[w] = v;
        s_idx[w] = i;
    }
    __syncthreads();
    v = s_val[0];
    i = s_idx[0];
    for (int q = 1; q < 4; ++q)
        if (cand_before(s_val[q], s_idx[q], v, i)) {
            v = s_val[q];
            i = s_idx[q];
        }
    __syncthreads();
}

// ctl = {steps done, slots done, this step is live, 0}
__global__ __launch_bounds__(256) void beam_select_partial_kernel(const float* __restrict__ logits, const float* __restrict__ bias, int nl,
                                                                 const float* __restrict__ scores, const uint8_t* __restrict__ done,
                                                                 const uint32_t* __restrict__ ctl, int R, int cur_beam, int V, int k,
                                                                 int C, int chunk, float* __restrict__ part_val,
                                                                 int64_t* __restrict__ part_idx) {
    __shared__ float red[4];
    __shared__ float s_val[4];
    __shared__ int64_t s_idx[4];
    if (ctl[1] >= (unsigned)R) return;      // every slot has finished: the search is frozen
    const int c = blockIdx.x, row = blockIdx.y;
    const float* xr = logits + (int64_t)row * V;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // (x - m) - lse with the reduction order of log_softmax_row_block_kernel (csrc/decoder.hip)
    float m = -INFINITY;
    for (int i = threadIdx.x; i < V; i += 256) m = fmaxf(m, xr[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (lane == 0) red[w] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int i = threadIdx.x; i < V; i += 256) sum += expf(xr[i] - m);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (lane == 0) red[w] = sum;
    __syncthreads();
    const float lse = logf((red[0] + red[1]) + (red[2] + red[3]));
    const float sc = scores[row];
    const bool masked = done && done[row];
    const float* br = bias ? bias + (int64_t)row * nl : nullptr;
    const int lo = c * chunk, hi = min(V, lo + chunk);
    const int64_t base = (int64_t)(row % cur_beam) * V;
    const int64_t out = ((int64_t)row * C + c) * k;
    float lv = BEAM_NONE_V;
    int64_t li = BEAM_NONE_I;
    for (int j = 0; j < k; ++j) {
        float best = BEAM_NONE_V;
        int64_t bi = BEAM_NONE_I;
        for (int i = lo + threadIdx.x; i < hi; i += 256) {
            float v = (xr[i] - m) - lse;      // the stored log-probability of the host path ...
            if (br && i < nl) v += br[i];     // ... its `logprobs[:, :nl] += lm_logprobs * lm_weight` ...
            v += sc;                          // ... and beam_topk_kernel's `lp[i] + row_score[row]`: three roundings
            if (masked) v = -INFINITY;
            const int64_t idx = base + i;
            if ((j == 0 || cand_before(lv, li, v, idx)) && cand_before(v, idx, best, bi)) {
                best = v;
                bi = idx;
            }
        }
        block_first(best, bi, s_val, s_idx);
        lv = best;
        li = bi;
        if (threadIdx.x == 0) {
            part_val[out + j] = lv;
            part_idx[out + j] = li;
        }
        if (li == BEAM_NONE_I) {               // the chunk is used up (uniform): the rest of its list is empty
            for (int q = j + 1 + threadIdx.x; q < k; q += 256) {
                part_val[out + q] = BEAM_NONE_V;
                part_idx[out + q] = BEAM_NONE_I;
            }
            break;
        }
    }
}

__global__ __launch_bounds__(256) void beam_select_merge_kernel(const float* __restrict__ part_val, const int64_t* __restrict__ part_idx,
                                                               uint32_t* __restrict__ ctl, int R, int n, int k,
                                                               float* __restrict__ sel_val, int64_t* __restrict__ sel_idx) {
    __shared__ float s_val[4];
    __shared__ int64_t s_idx[4];
    const bool live = ctl[1] < (unsigned)R;
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl[2] = live ? 1u : 0u;      // what this step's advance goes by
    if (!live) return;
    const int b = blockIdx.x;
    const float* pv = part_val + (int64_t)b * n;
    const int64_t* pi = part_idx + (int64_t)b * n;
    float lv = BEAM_NONE_V;
    int64_t li = BEAM_NONE_I;
    for (int j = 0; j < k; ++j) {
        float best = BEAM_NONE_V;
        int64_t bi = BEAM_NONE_I;
        for (int i = threadIdx.x; i < n; i += 256) {
            const float v = pv[i];
            const int64_t idx = pi[i];
            if ((j == 0 || cand_before(lv, li, v, idx)) && cand_before(v, idx, best, bi)) {
                best = v;
                bi = idx;
            }
        }
        block_first(best, bi, s_val, s_idx);
        lv = best;
        li = bi;
        if (threadIdx.x == 0) {
            sel_val[(int64_t)b * k + j] = lv != lv ? -INFINITY : lv;
            sel_idx[(int64_t)b * k + j] = li == BEAM_NONE_I ? 0 : li;      // (cannot happen: beam <= cur_beam * V candidates exist)
        }
    }
}

struct BeamState {
    uint32_t* ctl;
    float* scores;
    uint8_t* done;
    int32_t* rec_step;
    float* rec_score;
    int64_t* rec_tokens;
    const int64_t* tok_src;
    int64_t* tok_dst;
    const float* sel_val;
    const int64_t* sel_idx;
    float* spk_hist;
    int32_t* parent;
    int R, beam, V, ns, Lmax;
};

__global__ __launch_bounds__(256) void beam_advance_kernel(const BeamState p, int t, int n, int rep, int64_t terminate,
                                                          const float* __restrict__ spk, uint32_t* host, unsigned seq) {
    __shared__ int cnt_s[4];
    const int slot = blockIdx.x, tid = threadIdx.x;
    const bool live = p.ctl[2] != 0;
    if (live) {
        const int64_t idx = p.sel_idx[slot];
        const int src = (slot / p.beam) * p.beam + (int)(idx / p.V);
        const int64_t tok = idx % p.V;
        const int64_t* from = p.tok_src + (int64_t)src * n;
        int64_t* to = p.tok_dst + (int64_t)slot * (n + 1);
        for (int i = tid; i < n; i += 256) to[i] = from[i];
        const bool fin = terminate >= 0 && tok == terminate && !p.done[slot];      // (`done` belongs to the slot: system.py:203-215)
        if (fin) {
            int64_t* rec = p.rec_tokens + (int64_t)slot * p.Lmax;
            for (int i = tid; i < n; i += 256) rec[i] = from[i];
        }
        if (spk) {
            // step 0 on the seed rows: every slot of an item starts from the item's row (repeat_interleave, system.py:190);
            // later steps append row `slot` of this step's logits behind the history of the hypothesis the slot extends
            const float* sr = spk + (int64_t)(slot / rep) * p.ns;
            float* hr = p.spk_hist + ((int64_t)t * p.R + slot) * p.ns;
            for (int i = tid; i < p.ns; i += 256) hr[i] = sr[i];
        }
        __syncthreads();      // (every thread has read done[slot])
        if (tid == 0) {
            to[n] = tok;
            p.scores[slot] = p.sel_val[slot];
            if (spk) p.parent[(int64_t)t * p.R + slot] = src;
            if (fin) {
                p.rec_tokens[(int64_t)slot * p.Lmax + n] = tok;
                p.rec_step[slot] = t;
                p.rec_score[slot] = p.sel_val[slot];
                p.done[slot] = 1;
            }
        }
    }
    if (slot != 0) return;
    // slot 0's workgroup counts the finished slots from what this step selected: done' = done | (token == terminate), so a
    // flag another workgroup is setting right now gives the same count whichever value is read
    unsigned total = p.ctl[1];
    if (live) {
        int cnt = 0;
        for (int s = tid; s < p.R; s += 256)
            cnt += (p.done[s] || (terminate >= 0 && p.sel_idx[s] % p.V == terminate)) ? 1 : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
        if ((tid & 63) == 0) cnt_s[tid >> 6] = cnt;
        __syncthreads();
        total = (unsigned)((cnt_s[0] + cnt_s[1]) + (cnt_s[2] + cnt_s[3]));
        if (tid == 0) {
            p.ctl[1] = total;
            p.ctl[0] = (unsigned)(t + 1);
        }
    }
    if (host && tid == 0) {
        // pinned host memory mapped into the device's address space: the host looks at the counter without waiting for the stream
        __hip_atomic_store(host, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __threadfence_system();
        __hip_atomic_store(host + 1, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ __launch_bounds__(256) void beam_init_kernel(const int64_t* __restrict__ generated, int beam, int L0, int64_t* __restrict__ tok0,
                                                       int32_t* __restrict__ rec_step) {
    const int slot = blockIdx.x;
    for (int i = threadIdx.x; i < L0; i += 256) tok0[(int64_t)slot * L0 + i] = generated[(int64_t)(slot / beam) * L0 + i];
    if (threadIdx.x == 0) rec_step[slot] = -1;
}

// history of the hypothesis in `slot` after step `step`: position `pos` lives in the row reached by following the parent rows
// from step `step` down to `pos`
__global__ __launch_bounds__(256) void beam_gather_spk_kernel(const float* __restrict__ spk_hist, const int32_t* __restrict__ parent,
                                                             const uint32_t* __restrict__ ctl, const int32_t* __restrict__ pairs,
                                                             int R, int ns, int length, float* __restrict__ out) {
    __shared__ int row_s;
    const int i = blockIdx.x, pos = blockIdx.y;
    const int slot = pairs[2 * i], step = pairs[2 * i + 1];
    if (slot < 0 || slot >= R || step < 0 || step >= (int)ctl[0] || pos > step) return;      // (only steps that were stored)
    if (threadIdx.x == 0) {
        int r = slot;
        for (int s = step; s > pos; --s) r = min(max(parent[(int64_t)s * R + r], 0), R - 1);
        row_s = r;
    }
    __syncthreads();
    const float* from = spk_hist + ((int64_t)pos * R + row_s) * ns;
    float* to = out + ((int64_t)i * length + pos) * ns;
    for (int q = threadIdx.x; q < ns; q += 256) to[q] = from[q];
}

}  // namespace tal

extern "C" size_t tal_beam_workspace_bytes(int B, int beam, int L0, int length, int V, int num_speakers) {
    BeamLayout l;
    return beam_layout(B, beam, L0, length, V, num_speakers, l) ? l.total : 0;
}

static int beam_check(const tal_beam_ctx* c, const char* who, BeamLayout& l) {
    TAL_CHECK_ARG(c, "%s: null context", who);
    TAL_CHECK_ARG(c->B > 0 && c->beam > 0 && c->L0 > 0 && c->length > 0 && c->V > 0 && c->num_speakers >= 0,
                  "%s: bad shape B=%d beam=%d L0=%d length=%d V=%d num_speakers=%d", who, c->B, c->beam, c->L0, c->length, c->V,
                  c->num_speakers);
    TAL_CHECK_ARG(c->beam <= TOPK_MAX, "%s: beam=%d exceeds %d", who, c->beam, TOPK_MAX);
    TAL_CHECK_ARG((int64_t)c->B * c->beam <= BEAM_ROWS_MAX,
                  "%s: B x beam = %lld rows exceed %d (beyond it the host path's log-softmax sums a row in another order)", who,
                  (long long)c->B * c->beam, BEAM_ROWS_MAX);
    TAL_CHECK_ARG(beam_layout(c->B, c->beam, c->L0, c->length, c->V, c->num_speakers, l), "%s: bad shape", who);
    TAL_CHECK_ARG(c->workspace && c->workspace_bytes >= l.total, "%s: workspace of %zu bytes, %zu needed", who,
                  c->workspace ? c->workspace_bytes : (size_t)0, l.total);
    return TAL_OK;
}

extern "C" int tal_beam_init_fwd(tal_beam_ctx* c, const int64_t* generated, void* stream) {
    BeamLayout l;
    if (int rc = beam_check(c, "tal_beam_init_fwd", l)) return rc;
    TAL_CHECK_ARG(generated, "tal_beam_init_fwd: null pointer");
    c->done_host_dev = nullptr;
    if (c->done_host) {
        void* alias = nullptr;
        if (hipHostGetDevicePointer(&alias, c->done_host, 0) != hipSuccess || !alias) {
            set_error("tal_beam_init_fwd: done_host is not mapped pinned host memory (%s)", hipGetErrorString(hipGetLastError()));
            return TAL_EINVAL;
        }
        c->done_host_dev = reinterpret_cast<uint32_t*>(alias);
        reinterpret_cast<volatile uint32_t*>(c->done_host)[0] = 0u;
        reinterpret_cast<volatile uint32_t*>(c->done_host)[1] = 0u;
    }
    char* w = reinterpret_cast<char*>(c->workspace);
    c->ctl = reinterpret_cast<uint32_t*>(w + l.ctl);
    c->scores = reinterpret_cast<float*>(w + l.scores);
    c->done = reinterpret_cast<uint8_t*>(w + l.done);
    c->rec_step = reinterpret_cast<int32_t*>(w + l.rec_step);
    c->rec_score = reinterpret_cast<float*>(w + l.rec_score);
    c->rec_tokens = reinterpret_cast<int64_t*>(w + l.rec_tokens);
    c->tokens[0] = reinterpret_cast<int64_t*>(w + l.tok0);
    c->tokens[1] = reinterpret_cast<int64_t*>(w + l.tok1);
    c->sel_val = reinterpret_cast<float*>(w + l.sel_val);
    c->sel_idx = reinterpret_cast<int64_t*>(w + l.sel_idx);
    c->part_val = reinterpret_cast<float*>(w + l.part_val);
    c->part_idx = reinterpret_cast<int64_t*>(w + l.part_idx);
    c->spk_hist = c->num_speakers > 0 ? reinterpret_cast<float*>(w + l.spk_hist) : nullptr;
    c->parent = c->num_speakers > 0 ? reinterpret_cast<int32_t*>(w + l.parent) : nullptr;
    c->state_bytes = l.state_end;
    c->seq = 0;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(w, 0, l.state_end, s) != hipSuccess) {
        set_error("tal_beam_init_fwd: hipMemsetAsync failed: %s", hipGetErrorString(hipGetLastError()));
        return TAL_EHIP;
    }
    hipLaunchKernelGGL(beam_init_kernel, dim3((unsigned)(c->B * c->beam)), dim3(256), 0, s, generated, c->beam, c->L0, c->tokens[0],
                       c->rec_step);
    TAL_CHECK_LAUNCH("tal_beam_init_fwd");
    return TAL_OK;
}

static int beam_step_check(const tal_beam_ctx* c, const char* who, int step, int cur_beam, BeamLayout& l) {
    if (int rc = beam_check(c, who, l)) return rc;
    TAL_CHECK_ARG(step >= 0 && step < c->length, "%s: step %d outside [0, %d)", who, step, c->length);
    TAL_CHECK_ARG(cur_beam == c->beam || (cur_beam == 1 && step == 0),
                  "%s: cur_beam=%d (the seed rows of step 0, or beam=%d)", who, cur_beam, c->beam);
    TAL_CHECK_ARG((int64_t)c->beam <= (int64_t)cur_beam * c->V, "%s: beam=%d exceeds the %d x %d candidates of an item", who, c->beam,
                  cur_beam, c->V);
    TAL_CHECK_ARG(c->ctl == reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(c->workspace) + l.ctl) && c->sel_idx && c->tokens[1],
                  "%s: the context has not been through tal_beam_init_fwd", who);
    return TAL_OK;
}

extern "C" int tal_beam_select_fwd(tal_beam_ctx* c, int step, int cur_beam, const float* logits, const float* bias, int nl,
                                   void* stream) {
    BeamLayout l;
    if (int rc = beam_step_check(c, "tal_beam_select_fwd", step, cur_beam, l)) return rc;
    TAL_CHECK_ARG(logits, "tal_beam_select_fwd: null pointer");
    TAL_CHECK_ARG(bias ? (nl > 0 && nl <= c->V) : nl == 0, "tal_beam_select_fwd: bias block of %d columns (V=%d)", nl, c->V);
    const int R = c->B * c->beam, rows = c->B * cur_beam, k = c->beam;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(beam_select_partial_kernel, dim3((unsigned)l.C, (unsigned)rows), dim3(256), 0, s, logits, bias, nl, c->scores,
                       cur_beam == c->beam ? c->done : nullptr, c->ctl, R, cur_beam, c->V, k, l.C, l.chunk, c->part_val, c->part_idx);
    TAL_CHECK_LAUNCH("tal_beam_select_fwd(partial)");
    hipLaunchKernelGGL(beam_select_merge_kernel, dim3((unsigned)c->B), dim3(256), 0, s, c->part_val, c->part_idx, c->ctl, R,
                       cur_beam * l.C * k, k, c->sel_val, c->sel_idx);
    TAL_CHECK_LAUNCH("tal_beam_select_fwd(merge)");
    return TAL_OK;
}

extern "C" int tal_beam_advance_fwd(tal_beam_ctx* c, int step, int cur_beam, int64_t terminate_token, const float* spk_logits,
                                    void* stream) {
    BeamLayout l;
    if (int rc = beam_step_check(c, "tal_beam_advance_fwd", step, cur_beam, l)) return rc;
    TAL_CHECK_ARG(!spk_logits || c->num_speakers > 0, "tal_beam_advance_fwd: speaker logits without num_speakers");
    BeamState p;
    p.ctl = c->ctl; p.scores = c->scores; p.done = c->done; p.rec_step = c->rec_step; p.rec_score = c->rec_score;
    p.rec_tokens = c->rec_tokens; p.tok_src = c->tokens[step & 1]; p.tok_dst = c->tokens[(step + 1) & 1];
    p.sel_val = c->sel_val; p.sel_idx = c->sel_idx; p.spk_hist = c->spk_hist; p.parent = c->parent;
    p.R = c->B * c->beam; p.beam = c->beam; p.V = c->V; p.ns = c->num_speakers; p.Lmax = c->L0 + c->length;
    c->seq += 1;
    hipLaunchKernelGGL(beam_advance_kernel, dim3((unsigned)p.R), dim3(256), 0, (hipStream_t)stream, p, step, c->L0 + step,
                       c->beam / cur_beam, terminate_token, spk_logits, c->done_host_dev, c->seq);
    TAL_CHECK_LAUNCH("tal_beam_advance_fwd");
    return TAL_OK;
}

extern "C" int tal_beam_gather_spk_fwd(const tal_beam_ctx* c, const int32_t* pairs, int n, float* out, void* stream) {
    BeamLayout l;
    if (int rc = beam_check(c, "tal_beam_gather_spk_fwd", l)) return rc;
    TAL_CHECK_ARG(c->num_speakers > 0 && c->spk_hist && c->parent, "tal_beam_gather_spk_fwd: the context keeps no speaker history");
    TAL_CHECK_ARG(n >= 0 && (n == 0 || (pairs && out)), "tal_beam_gather_spk_fwd: bad argument");
    if (n == 0) return TAL_OK;
    hipLaunchKernelGGL(beam_gather_spk_kernel, dim3((unsigned)n, (unsigned)c->length), dim3(256), 0, (hipStream_t)stream, c->spk_hist,
                       c->parent, c->ctl, pairs, c->B * c->beam, c->num_speakers, c->length, out);
    TAL_CHECK_LAUNCH("tal_beam_gather_spk_fwd");
    return TAL_OK;
}
