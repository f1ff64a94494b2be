// The decode step of System.generate_unaligned (tal/asr/system.py:332-411) as ONE launch: G persistent workgroups per session walk
// the step's phases -- embed, per decoder layer {q | k | v^T, self-attention, out-projection + ReZero, cross q, key-split
// cross-attention, out-projection + ReZero, FFN-1, FFN-2 cut along K}, LM head + pick -- and call, for the blocks dealt to them, the
// SAME device bodies the launch chain's kernels run (csrc/decode_bodies.h) with the same arguments: every token, attention row and
// hidden state is bit-identical to tal_greedy_step_fwd's chain of 34 launches.  What changes is what sits between two phases: a
// counter barrier among the session's workgroups instead of a kernel boundary.
//
// Hand-off protocol (the MI355X guide's recipe R1, priced in profiles/r5_decode_persistent_skeleton.txt): a phase's outputs are
// stored write-through at agent scope (the bodies' COH form); every wave drains its stores (s_waitcnt vmcnt(0)), the workgroup
// meets at its own barrier, ONE lane adds 1 to the session's arrival counter (agent scope, relaxed) and polls it (relaxed load +
// s_sleep) until phase x G workgroups have arrived; then ONE lane issues an agent-scope acquire fence (the CU's L1 and the L2's
// non-local lines are dropped) and the workgroup's plain loads of the next phase are fresh.  Counters live in the session's ticket
// block (words PS_BAR, PS_DONE; PS_ERR is raised when a wait gives up) and are left at zero by the launch, like the other tickets.
// Sessions are independent: several of them (the decode sessions of System.transcribe_unaligned_many) run side by side in one
// launch, G workgroups each, without ever waiting for one another.
#include "decode_bodies.h"

namespace tal {

// (ablation build -DPS_TIMELINE: workgroups 0 and G - 1 of session 0 stamp the 100 MHz wall clock around every phase barrier;
//  scripts/decode_persist_timeline.py reads them through tal_debug_ps_timeline.  Not part of the product library.)
#ifdef PS_TIMELINE
__device__ unsigned long long g_ps_tl[2 * 64 * 4];
#define PS_STAMP(b, i)                                                                                         \
    do {                                                                                                       \
        if (threadIdx.x == 0 && (b).tl >= 0 && (b).phase < 64) g_ps_tl[((b).tl * 64 + (b).phase) * 4 + (i)] = wall_clock64(); \
    } while (0)
#else
#define PS_STAMP(b, i)
#endif

struct PsBarrier {
    unsigned* bar;
    unsigned* err;
    unsigned G, phase;
    int tl;
    float* out;              // the session's result buffer {token, row [S] (, sequence word)}: receives the failure marker
    int S;
    unsigned host_seq;
    bool wg0;                // the session's first workgroup: writes the marker whenever it sees the step fail
};
// A step that cannot finish (a barrier wait gave up: its workgroups were not resident together, or one of them died) must not look
// like a step that did: the FIRST workgroup to raise the error word writes the token -1 and, for a host-polled step, the sequence
// word, so that the host's poll returns and finds the marker (tal_greedy_step_fwd / tal_greedy_step_poll then report TAL_EHIP and
// the context's ticket block -- phase counters, error word, half-counted attention / split-K tickets -- is zeroed before its next
// step).  Every workgroup checks the error word before, inside and after its wait, so none runs a phase behind a failed barrier;
// the session's first workgroup writes the marker too when it finds the word raised (a word left raised by an earlier failure
// has no first raiser in this launch).
__device__ __forceinline__ void ps_mark(PsBarrier& b) {
    __hip_atomic_store(reinterpret_cast<unsigned*>(b.out), 0xffffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (b.host_seq) __hip_atomic_store(reinterpret_cast<unsigned*>(b.out + 1 + b.S), b.host_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void ps_raise(PsBarrier& b) {
    if (__hip_atomic_exchange(b.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) ps_mark(b);      // (the first to raise it)
}
// -> false: a wait gave up (or another workgroup's did): the caller leaves the kernel without delivering a result
__device__ __forceinline__ bool ps_sync(PsBarrier& b) {
    __shared__ unsigned ok_sh;
    PS_STAMP(b, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // every wave: its write-through stores are acknowledged
    __syncthreads();
    PS_STAMP(b, 1);
    if (threadIdx.x == 0) {
        ++b.phase;
        __hip_atomic_fetch_add(b.bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned target = b.phase * b.G;
        const long long t0 = wall_clock64();
        // (the error word is looked at before the wait too: a counter left at or beyond the target by a step that failed earlier
        //  would let every wait fall through without ordering anything)
        unsigned ok = __hip_atomic_load(b.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u ? 1u : 0u;
        while (ok && __hip_atomic_load(b.bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            __builtin_amdgcn_s_sleep(1);
            if (wall_clock64() - t0 > 20000000ll) {                                     // 200 ms at 100 MHz
                ps_raise(b);
                ok = 0u;
            } else if (__hip_atomic_load(b.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                ok = 0u;
            }
        }
        if (ok && __hip_atomic_load(b.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) ok = 0u;
        if (!ok && b.wg0) ps_mark(b);
#ifdef PS_TIMELINE
        --b.phase; PS_STAMP(b, 2); ++b.phase;
#endif
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        ok_sh = ok;
    }
    __syncthreads();
#ifdef PS_TIMELINE
    --b.phase; PS_STAMP(b, 3); ++b.phase;
#endif
    return ok_sh != 0u;
}

template <int MODE>
__device__ __forceinline__ void ps_skinny(const SkinnyArgs& g, unsigned wg, unsigned G) {
    const unsigned gx = (unsigned)(g.N / 16), gy = (unsigned)((g.M + 31) / 32), gz = (unsigned)(g.ksplit > 1 ? g.ksplit : 1);
    for (unsigned vb = wg; vb < gx * gy * gz; vb += G) {
        const Blk blk{vb % gx, (vb / gx) % gy, vb / (gx * gy), gx, gy};
        if (g.M <= 16) skinny_gemm_body<MODE, 1, 4, true>(g, blk);
        else skinny_gemm_body<MODE, 2, 4, true>(g, blk);
        __syncthreads();          // (the body's LDS buffers are reused by the next block)
    }
}

// a session's view of layer l (batch 1, no target mask, the last row's per-head probabilities; no folded-layer buffers)
__device__ __forceinline__ LayerIo ps_layer_io(const PsSession& s, int l, const float* cur, int H) {
    LayerIo x = {};
    x.tgt = cur; x.out = s.h1; x.B = 1; x.U = s.U; x.S = s.S;
    x.qkv = s.qkv; x.vt = s.vt; x.ctx = s.ctx; x.x1 = s.x1; x.x2 = s.x2; x.ff = s.ff;
    x.ck = s.k_cache[l]; x.k_pitch = s.k_pitch; x.cvt = s.vt_cache[l]; x.kpm = s.kpm;
    x.probs = s.probs + (size_t)l * H * s.S; x.prob_row0 = s.U - 1;
    x.sk_part = s.sk_part; x.tickets = s.tickets;
    return x;
}

template <int HD>
__global__ __launch_bounds__(256) void greedy_persist_kernel(const PsArgs a) {
    const unsigned G = (unsigned)a.G;
    const unsigned si = blockIdx.x / G, wg = blockIdx.x - si * G;
    const PsSession& s = a.s[si];
    const PsModel& m = a.m;
    const int E = m.E, H = m.H, U = s.U, S = s.S, K0 = m.K0;
    const LayerDims d{E, H, m.FF, m.qscale};
    PsBarrier bar{s.tickets + PS_BAR, s.tickets + PS_ERR, G, 0u, si == 0 ? (wg == 0 ? 0 : (wg == G - 1 ? 1 : -1)) : -1, s.out, S, s.host_seq, wg == 0};

    // ---- embed (models.py:218-223)
    for (unsigned row = wg; row < (unsigned)U; row += G) {
        embed_body<true>(s.tokens, m.emb, m.proj, m.pe, s.h0, U, m.V, K0, E, (int)row);
        __syncthreads();
    }
    if (!ps_sync(bar)) return;

    // ---- the UNFOLDED layer's phases, each on the arguments the launch chain builds (csrc/decode_bodies.h)
    const float* cur = s.h0;
    for (int l = 0; l < m.n_layers; ++l) {
        const tal_decoder_layer_w& w = m.layer[l];
        const LayerIo x = ps_layer_io(s, l, cur, H);
        ps_skinny<3>(sa_qkv(w, x, d), wg, G);
        if (!ps_sync(bar)) return;
        {
            const AttnArgs t = sa_attn(x, d);
            const unsigned gx = (unsigned)((U + 15) / 16);
            for (unsigned vb = wg; vb < gx * (unsigned)H; vb += G) {
                attn_small_body<HD, 4, true>(t, Blk{vb % gx, vb / gx, 0u, gx, (unsigned)H});
                __syncthreads();
            }
        }
        if (!ps_sync(bar)) return;
        ps_skinny<2>(sa_out(w, x, d), wg, G);
        if (!ps_sync(bar)) return;
        ps_skinny<3>(ca_q(w, x, d), wg, G);
        if (!ps_sync(bar)) return;
        {
            const AttnArgs c = ca_attn(w, x, d, false);
            const int CB = split_cb(S), nblk = (S + 15) / 16, NCH = (nblk + CB - 1) / CB;
            const unsigned gx = (unsigned)((U + 15) / 16);
            for (unsigned vb = wg; vb < gx * (unsigned)H * (unsigned)NCH; vb += G) {
                attn_split_body<HD, true>(c, CB, NCH, x.sk_part, x.tickets, Blk{vb % gx, (vb / gx) % (unsigned)H, vb / (gx * (unsigned)H), gx, (unsigned)H});
                __syncthreads();
            }
        }
        if (!ps_sync(bar)) return;
        ps_skinny<2>(ca_out(w, x, d), wg, G);
        if (!ps_sync(bar)) return;
        ps_skinny<1>(ff1(w, x, d), wg, G);
        if (!ps_sync(bar)) return;
        ps_skinny<2>(ff2(w, x, d, false, true), wg, G);
        if (!ps_sync(bar)) return;
        cur = s.h1;
    }
    // ---- tied factorised LM head on the last position + pick + the new token's attention row (models.py:243-246, system.py:355-411)
    {
        // (no bias: a context with an LM row does not take the one-launch form: greedy_persist_ok)
        const LmPickArgs q = lm_pick_args(cur + (size_t)(U - 1) * E, s.probs, (int64_t)H * S, (int64_t)S, S, s.pick_part, s.tickets, s.out,
                                          s.token_out, s.host_seq, nullptr);
        const unsigned gx = (unsigned)((m.V + LMP_ROWS - 1) / LMP_ROWS);
        for (unsigned bx = wg; bx < gx; bx += G) {
            lm_pick_body(q, m.proj_t, E, K0, m.emb, m.V, m.n_layers, H, bx, gx);
            __syncthreads();
        }
    }
    // ---- the counters go back to zero behind the last workgroup (every workgroup is past every wait by then)
    if (threadIdx.x == 0) {
        const unsigned d = __hip_atomic_fetch_add(s.tickets + PS_DONE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (d == G - 1) {
            __hip_atomic_store(s.tickets + PS_BAR, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(s.tickets + PS_DONE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// dynamic LDS of the launch: the largest of its phases' (embedding row | self-attention scores | cross-attention chunk | pick)
static size_t ps_lds_bytes(const PsArgs& a) {
    size_t n = (size_t)a.m.K0;
    const size_t pick = (size_t)a.m.E + a.m.K0 + LMP_ROWS;
    n = pick > n ? pick : n;
    for (int i = 0; i < a.n; ++i) {
        const size_t self = (size_t)16 * (((a.s[i].U + 15) & ~15) + 4);
        const size_t cross = (size_t)16 * (split_cb(a.s[i].S) * 16 + 4);
        n = self > n ? self : n;
        n = cross > n ? cross : n;
    }
    return n * sizeof(float);
}

int launch_greedy_persist(const PsArgs& a, hipStream_t s) {
    TAL_CHECK_ARG(a.n >= 1 && a.n <= TAL_PS_MAX_SESS && a.G >= 1, "one-launch decode step: %d sessions x %d workgroups", a.n, a.G);
    TAL_CHECK_ARG(a.n * a.G <= device_cus(), "one-launch decode step: %d workgroups must be resident together on %d CUs", a.n * a.G, device_cus());
    const int hd = a.m.E / a.m.H;
    const size_t lds = ps_lds_bytes(a);
    TAL_CHECK_ARG(lds <= 48 * 1024, "one-launch decode step: %zu bytes of LDS", lds);
    const dim3 grid((unsigned)(a.n * a.G));
    double work = 0.0;
    for (int i = 0; i < a.n; ++i) work += 2.0 * a.s[i].U * (double)a.m.n_layers * ((double)a.m.E * (6.0 * a.m.E + 2.0 * a.m.FF));
    ProfScope prof(PROF_OTHER, work, s);
    switch (hd) {
        case 128: hipLaunchKernelGGL((greedy_persist_kernel<128>), grid, dim3(256), lds, s, a); break;
        case 64: hipLaunchKernelGGL((greedy_persist_kernel<64>), grid, dim3(256), lds, s, a); break;
        default:
            set_error("one-launch decode step: head dimension %d not built", hd);
            return TAL_EINVAL;
    }
    TAL_CHECK_LAUNCH("one-launch decode step");
    return TAL_OK;
}

}  // namespace tal

#ifdef PS_TIMELINE
extern "C" int tal_debug_ps_timeline(void* host_out) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(tal::g_ps_tl), sizeof(tal::g_ps_tl)) == hipSuccess ? 0 : -3;
}
#endif
