// plan_main.cpp -- carma_mband_smooth_plan.h (the host-only planner of carma_bands_smooth) as a stand-alone program; test harness.
//   plan_main times t0           stdin: M, the M requested times -> 2 lines: perm, the (M + 1) x 4 record values
//   plan_main strides p ng       -> one line: fields fs ps ws
//   plan_main chunks p ng B c [cap]  -> one line: rows waves chunks bytes     (c <= 0: automatic; cap: bytes, default the library's)
//   plan_main check h K N theta B band tout M mean var bmean bvar [bad]
//        h, theta, tout, mean, var, bmean, bvar: 0 = NULL, 1 = given; bad: index of a requested time set to NaN (-1: none),
//        bad = -2: +inf at index 0 -> the message, or an empty line
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../carma_pack_amd/csrc/carma_mband_smooth_plan.h"

int main(int argc, char** argv)
{
    using namespace carma;
    if (argc == 3 && !strcmp(argv[1], "times")) {
        int M = 0;
        if (scanf("%d", &M) != 1 || M < 1) return 2;
        std::vector<double> tout(M);
        for (double& v : tout)
            if (scanf("%lf", &v) != 1) return 2;
        const MbandSmoothTimes s = mband_smooth_times(tout.data(), M, atof(argv[2]));
        if ((int)s.perm.size() != M || s.rec.size() != 4 * ((size_t)M + 1)) return 3;
        for (int v : s.perm) printf("%d ", v);
        printf("\n");
        for (double v : s.rec) printf("%.17g ", v);
        printf("\n");
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "strides")) {
        const MbandSmoothStrides s = mband_smooth_strides(atoi(argv[2]), atoi(argv[3]));
        printf("%d %ld %ld %zu\n", s.fields, s.fs, s.ps, s.ws);
        return 0;
    }
    if ((argc == 6 || argc == 7) && !strcmp(argv[1], "chunks")) {
        const MbandSmoothChunks c = argc == 7 ? mband_smooth_chunks(atoi(argv[2]), atoi(argv[3]), atol(argv[4]), atol(argv[5]),
                                                                    (size_t)atoll(argv[6]))
                                              : mband_smooth_chunks(atoi(argv[2]), atoi(argv[3]), atol(argv[4]), atol(argv[5]));
        printf("%ld %ld %ld %zu\n", c.rows, c.waves, c.chunks, c.bytes);
        return 0;
    }
    if ((argc == 14 || argc == 15) && !strcmp(argv[1], "check")) {
        const int M = atoi(argv[9]);
        std::vector<double> tout(M > 0 ? M : 1, 1.5), buf(4, 0.0);
        const int bad = argc == 15 ? atoi(argv[14]) : -1;
        if (bad >= 0 && bad < M) tout[bad] = std::nan("");
        if (bad == -2) tout[0] = std::numeric_limits<double>::infinity();
        auto ptr = [&](const char* s, double* p) { return atoi(s) ? p : nullptr; };
        const std::string msg =
            mband_smooth_check(atoi(argv[2]) != 0, atoi(argv[3]), atol(argv[4]), ptr(argv[5], buf.data()), atoi(argv[6]), atoi(argv[7]),
                               ptr(argv[8], tout.data()), M, ptr(argv[10], buf.data()), ptr(argv[11], buf.data() + 1),
                               ptr(argv[12], buf.data() + 2), ptr(argv[13], buf.data() + 3));
        printf("%s\n", msg.c_str());
        return 0;
    }
    fprintf(stderr, "usage: plan_main times t0 | strides p ng | chunks p ng B c [cap] | check ...\n");
    return 1;
}
