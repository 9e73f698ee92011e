// plan_main.cpp -- carma_mband_set_smooth_plan.h (the host-only planner of carma_bandset_smooth) and MbandSet::t0
// (carma_mband_set_plan.h) as a stand-alone program; test harness.  Everything but the mode comes from stdin.
//   plan_main plan p forced cap     S, nobj [S], t0 [S], B, toff[0], then per row: object band M and the M times
//        -> lines: "W J sc_max", wave_job, job_obj, job_band, job_M, job_req, row_idx, wave_sc, out_off, chunk0, req
//        (cap: bytes; <= 0: the library's)
//   plan_main check                 h S K, nobj [S], B, mask, object [B], band [B], toff [B + 1], n, tout [n]
//        mask: bit 0 ... 6 set = theta, object, band, tout, toff, mean, var is NULL -> the message, or an empty line
//   plan_main t0                    S K, offsets [S K + 1], then time, y, yerr [offsets[S K]] each
//        -> 2 lines: MbandSet::t0 of the set, MbandObject::t0 of every object prepared alone
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../carma_pack_amd/csrc/carma_mband_set_plan.h"
#include "../../carma_pack_amd/csrc/carma_mband_set_smooth_plan.h"

template <class T>
static void line(const std::vector<T>& v)
{
    for (const T& x : v) printf("%ld ", (long)x);
    printf("\n");
}

static bool rd(int& v) { return scanf("%d", &v) == 1; }
static bool rd(long& v) { return scanf("%ld", &v) == 1; }
static bool rd(double& v) { return scanf("%lf", &v) == 1; }
template <class T>
static bool rd(std::vector<T>& v)
{
    for (T& x : v)
        if (!rd(x)) return false;
    return true;
}

int main(int argc, char** argv)
{
    using namespace carma;
    if (argc == 5 && !strcmp(argv[1], "plan")) {
        int S = 0, B = 0;
        long toff0 = 0;
        if (!rd(S) || S < 1) return 2;
        std::vector<int> nobj(S);
        std::vector<double> t0(S);
        if (!rd(nobj) || !rd(t0) || !rd(B) || B < 1 || !rd(toff0) || toff0 < 0) return 2;
        std::vector<int> object(B), band(B);
        std::vector<long> toff(1, toff0);
        std::vector<double> tout((size_t)toff0, -777.0);       // (never read: the rows start at toff[0])
        for (int i = 0; i < B; i++) {
            int M = 0;
            if (!rd(object[i]) || !rd(band[i]) || !rd(M) || M < 1) return 2;
            std::vector<double> t(M);
            if (!rd(t)) return 2;
            tout.insert(tout.end(), t.begin(), t.end());
            toff.push_back(toff.back() + M);
        }
        const long cap = atol(argv[4]);
        const MbandSetSmoothPlan pl = cap > 0 ? mbandset_smooth_plan(atoi(argv[2]), object.data(), band.data(), B, tout.data(), toff.data(),
                                                                     nobj.data(), t0.data(), atol(argv[3]), (size_t)cap)
                                              : mbandset_smooth_plan(atoi(argv[2]), object.data(), band.data(), B, tout.data(), toff.data(),
                                                                     nobj.data(), t0.data(), atol(argv[3]));
        printf("%ld %ld %zu\n", pl.W, pl.J, pl.sc_max);
        line(pl.wave_job);
        line(pl.job_obj);
        line(pl.job_band);
        line(pl.job_M);
        line(pl.job_req);
        line(pl.row_idx);
        line(pl.wave_sc);
        line(pl.out_off);
        line(pl.chunk0);
        for (double v : pl.req) printf("%.17g ", v);
        printf("\n");
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "check")) {
        int h = 0, S = 0, K = 0, B = 0, mask = 0, n = 0;
        if (!rd(h) || !rd(S) || !rd(K) || S < 0) return 2;
        std::vector<int> nobj(S);
        if (!rd(nobj) || !rd(B) || !rd(mask)) return 2;
        const int nb = B > 0 ? B : 0;
        std::vector<int> object(nb), band(nb);
        std::vector<long> toff((size_t)nb + 1);
        if (!rd(object) || !rd(band) || !rd(toff) || !rd(n) || n < 0) return 2;
        std::vector<double> tout(n), buf(3, 0.0);
        if (!rd(tout)) return 2;
        auto have = [&](int bit) { return !(mask & (1 << bit)); };
        const std::string msg = mbandset_smooth_check(h != 0, S, K, nobj.data(), have(0) ? buf.data() : nullptr,
                                                      have(1) ? object.data() : nullptr, have(2) ? band.data() : nullptr, B,
                                                      have(3) ? tout.data() : nullptr, have(4) ? toff.data() : nullptr,
                                                      have(5) ? buf.data() + 1 : nullptr, have(6) ? buf.data() + 2 : nullptr);
        printf("%s\n", msg.c_str());
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "t0")) {
        int S = 0, K = 0;
        if (!rd(S) || !rd(K) || S < 1 || K < 1 || K > MBAND_PLAN_KMAX) return 2;
        std::vector<long> off((size_t)S * K + 1);
        if (!rd(off)) return 2;
        std::vector<double> t((size_t)off.back()), y(t.size()), e(t.size());
        if (!rd(t) || !rd(y) || !rd(e)) return 2;
        const std::vector<double> lo((size_t)S * K, -1.0), hi((size_t)S * K, 1.0);
        MbandSet m;
        if (mbandset_prepare(t.data(), y.data(), e.data(), off.data(), S, K, lo.data(), hi.data(), nullptr, m) >= 0) return 3;
        for (double v : m.t0) printf("%.17g ", v);
        printf("\n");
        for (int s = 0; s < S; s++) {
            long loc[MBAND_PLAN_KMAX + 1];
            mbandset_object_offsets(off.data(), s, K, loc);
            const long base = off[(size_t)s * K];
            MbandObject o;
            if (!mband_prepare(t.data() + base, y.data() + base, e.data() + base, loc, K, lo.data(), hi.data(), nullptr, o)) return 3;
            printf("%.17g ", o.t0);
        }
        printf("\n");
        return 0;
    }
    fprintf(stderr, "usage: plan_main plan p forced cap | check | t0   (the data on stdin)\n");
    return 1;
}
