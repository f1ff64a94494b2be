// csrc/head_plan.h on the host: the run partition of the streaming heads over a grid of shapes and grid overrides.  Checks what
// the merge kernels rely on (one partial per lane: a row block never meets more than hp <= 16 workgroups) and that block_of is
// the inverse of the runs.  Prints the number of combinations and the largest hp seen; exits non-zero at the first violation.
#include <stdio.h>
#include <stdlib.h>

#include "../tal_asrd_amd/csrc/head_plan.h"

using namespace tal;

#define CHECK(cond)                                                                                                        \
    do {                                                                                                                   \
        if (!(cond)) {                                                                                                     \
            printf("FAILED %s: bn=%d wgs=%d M=%lld S=%d override=%lld grid=%lld hp=%d\n", #cond, bn, wgs, (long long)M, S,   \
                   (long long)ov, (long long)G, p.hp);                                                                    \
            return 1;                                                                                                      \
        }                                                                                                                  \
    } while (0)

int main() {
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
                        CHECK(G >= 1);
                        CHECK(p.hp >= 1 && p.hp <= SLOTS);
                        const int64_t blocks[] = {0, MB > 1 ? 1 : 0, MB / 2, MB - 1};
                        for (int64_t m : blocks) {
                            const int64_t met = block_of(m * NT + NT - 1, U, G) - block_of(m * NT, U, G) + 1;
                            CHECK(met >= 1 && met <= p.hp);
                        }
                        // the runs [b U / G, (b + 1) U / G) are non-empty, adjacent, cover [0, U), and block_of maps both ends of
                        // run b (hence, being monotonic, everything between) back to b
                        int64_t next = 0;
                        for (int64_t b = 0; b < G; ++b) {
                            const int64_t u0 = b * U / G, u1 = (b + 1) * U / G;
                            CHECK(u0 == next && u1 > u0);
                            CHECK(block_of(u0, U, G) == b && block_of(u1 - 1, U, G) == b);
                            next = u1;
                        }
                        CHECK(next == U);
                        worst = p.hp > worst ? p.hp : worst;
                        ++combos;
                    }
    printf("combinations %ld worst_hp %d\n", combos, worst);
    return 0;
}
