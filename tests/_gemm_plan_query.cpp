// csrc/gemm_plan.h on the host, one call per line of stdin (tests/test_dense_forms_cpu.py): a TDS layer as launch_linear_f16x3 passes
// it -- the fp16x3 form, packed rows, 16-byte pointers, one batch.  Line:
//   cus M N K mode out_split res_split has_range_flag ws_bytes  s64_below no_w64 no_glds no_splitk4 no_splitk_tail no_row_split no_n96
//   global_loads s64_rows s64_order w64_stagger
// Output per call: one "S <kernel> rows row0 bm bn waves n_major tiles_m tiles_n grid_x split" line per step, then "E <steps>" ("E -1":
// refused).
#include <stdio.h>

#include "../tal_asrd_amd/csrc/gemm_plan.h"

using namespace tal;

int main() {
    long long M, ws;
    int cus, N, K, mode, out_split, res_split, flag, o[11];
    for (;;) {
        const int got = scanf("%d %lld %d %d %d %d %d %d %lld %d %d %d %d %d %d %d %d %d %d %d", &cus, &M, &N, &K, &mode, &out_split, &res_split, &flag, &ws,
                              &o[0], &o[1], &o[2], &o[3], &o[4], &o[5], &o[6], &o[7], &o[8], &o[9], &o[10]);
        if (got == EOF) return 0;
        if (got != 20) {
            fprintf(stderr, "bad line: %d fields\n", got);
            return 1;
        }
        GemmCall c = {};
        c.M = M; c.N = N; c.K = K; c.mode = mode; c.nbatch = 1;
        c.f16x3 = true; c.out_split = out_split != 0; c.res_split = res_split != 0; c.has_range_flag = flag != 0;
        c.lda = K; c.ldw = K; c.ldy = N; c.ldres = N;
        c.has_ws = ws > 0; c.splitk_ws_bytes = (size_t)ws;
        c.cus = cus;
        c.o.s64_below = o[0]; c.o.no_w64 = o[1]; c.o.no_glds = o[2]; c.o.no_splitk4 = o[3]; c.o.no_splitk_tail = o[4]; c.o.no_row_split = o[5];
        c.o.no_n96 = o[6]; c.o.global_loads = o[7]; c.o.s64_rows = o[8]; c.o.s64_order = o[9]; c.o.w64_stagger = o[10];
        const GemmPlan p = gemm_plan(c);
        if (p.grid_too_large) {
            printf("E -1\n");
            continue;
        }
        for (int i = 0; i < p.n; ++i) {
            const GemmStep& st = p.step[i];
            const char* name = st.kernel == GK_S64 ? "s64" : st.kernel == GK_W64 ? "w64" : st.kernel != GK_GLDS ? "other" : st.bn == 160 ? "glds160" : "glds96";
            printf("S %s %lld %lld %d %d %d %d %d %d %u %d\n", name, (long long)st.rows, (long long)st.row0, st.bm, st.bn, st.waves, st.n_major, st.tiles_m,
                   st.tiles_n, st.grid_x, st.split);
        }
        printf("E %d\n", p.n);
    }
}
