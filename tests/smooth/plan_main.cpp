// plan_main.cpp -- carma_smooth_plan.h (the host-only planner of the one-pass smoother) as a stand-alone program; test harness.
//   plan_main merge            stdin: n M, the n data times, the M requested times -> 4 lines: grid, dpos, spos, src
//   plan_main chunks G ng K c  -> one line: E models waves rec_elems grp_elems bytes   (G = 0: CAR(1); c <= 0: automatic)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../carma_pack_amd/csrc/carma_smooth_plan.h"

int main(int argc, char** argv)
{
    using namespace carma;
    if (argc >= 2 && !strcmp(argv[1], "merge")) {
        int n = 0, M = 0;
        if (scanf("%d %d", &n, &M) != 2 || n < 0 || M < 0) return 2;
        std::vector<double> t(n), tout(M);
        for (double& v : t)
            if (scanf("%lf", &v) != 1) return 2;
        for (double& v : tout)
            if (scanf("%lf", &v) != 1) return 2;
        const SmoothGrid g = smooth_merge(t.data(), n, tout.data(), M);
        if (g.ng != n + M || (int)g.grid.size() != g.ng || (int)g.src.size() != g.ng) return 3;
        for (double v : g.grid) printf("%.17g ", v);
        printf("\n");
        for (int v : g.dpos) printf("%d ", v);
        printf("\n");
        for (int v : g.spos) printf("%d ", v);
        printf("\n");
        for (int v : g.src) printf("%d ", v);
        printf("\n");
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "chunks")) {
        const SmoothChunks c = smooth_chunks(atoi(argv[2]), atoi(argv[3]), atol(argv[4]), atol(argv[5]));
        printf("%d %ld %ld %zu %zu %zu\n", c.E, c.models, c.waves, c.rec_elems, c.grp_elems, c.bytes);
        return 0;
    }
    fprintf(stderr, "usage: plan_main merge | plan_main chunks G ng K c\n");
    return 1;
}
