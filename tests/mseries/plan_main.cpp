// plan_main.cpp -- carma_mseries_plan.h (the host-only launch planners of the multi-series calls) as a stand-alone program; test
// harness.  A case comes in on stdin as whitespace-separated numbers, the tables go out as lines "name v v v ...".
//   plan_main logdens   S B, nser[S], repdt[S], series[B]          -> bad i | W w_plain cnt first order used wave_series eval_idx
//   plan_main filter    S M, nser[S], series[M]                    -> W tile_total nmax offs order tint tlong
//   plan_main predict   G S M, nser[S], series[M], toff[M + 1]     -> W T E tint tlong                    (G = 0: CAR(1))
//   plan_main smooth    G S M forced, nser[S], the data times of all series, series[M], toff[M + 1], tout[toff[M]]
//                                                                   -> E W J pts_max chunk0 tint tlong grids
//   plan_main toff      M, toff[M + 1]                              -> toff r      (r as check_toff returns it)
//   plan_main chunk     nmax                                        -> chunk c     (c = mpt_chunk_iters(nmax))
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../carma_pack_amd/csrc/carma_mseries_plan.h"

template <class T>
static bool rd(std::vector<T>& v)
{
    for (T& x : v) {
        double d;
        if (scanf("%lf", &d) != 1) return false;
        x = (T)d;
    }
    return true;
}

template <class T>
static void put(const char* name, const T* v, size_t n)
{
    printf("%s", name);
    for (size_t i = 0; i < n; i++) printf(" %lld", (long long)v[i]);
    printf("\n");
}
template <class T>
static void put(const char* name, const std::vector<T>& v) { put(name, v.data(), v.size()); }
static void put1(const char* name, long long v) { printf("%s %lld\n", name, v); }

int main(int argc, char** argv)
{
    using namespace carma;
    if (argc != 2) {
        fprintf(stderr, "usage: plan_main logdens | filter | predict | smooth | toff | chunk   (the case on stdin)\n");
        return 1;
    }
    const char* mode = argv[1];
    if (!strcmp(mode, "toff")) {
        int M = 0;
        if (scanf("%d", &M) != 1 || M < 0) return 2;
        std::vector<long> toff((size_t)M + 1);
        if (!rd(toff)) return 2;
        put1("toff", check_toff(toff.data(), M));
        return 0;
    }
    if (!strcmp(mode, "chunk")) {
        int nmax = 0;
        if (scanf("%d", &nmax) != 1) return 2;
        put1("chunk", mpt_chunk_iters(nmax));
        return 0;
    }
    if (!strcmp(mode, "logdens")) {
        int S = 0, B = 0;
        if (scanf("%d %d", &S, &B) != 2 || S < 1 || B < 0) return 2;
        std::vector<int> nser(S), series(B);
        std::vector<char> repdt(S);
        if (!rd(nser) || !rd(repdt) || !rd(series)) return 2;
        MlogdensPlan pl;
        for (int rep = 0; rep < 2; rep++) {                   // twice: the second call runs on a used workspace
            const long bad = mlogdens_plan_count(series.data(), B, S, nser.data(), repdt.data(), pl);
            if (bad >= 0) {
                put1("bad", bad);
                return 0;
            }
        }
        std::vector<int> wser((size_t)pl.W, -7), eidx((size_t)pl.W * 64, -7);
        mlogdens_plan_fill(pl, wser.data(), eidx.data());
        put1("W", pl.W);
        put1("w_plain", pl.w_plain);
        put("cnt", pl.b.cnt);
        put("first", pl.b.first);
        put("order", pl.b.order);
        put("used", pl.used);
        put("wave_series", wser);
        put("eval_idx", eidx);
        return 0;
    }
    if (!strcmp(mode, "filter")) {
        int S = 0, M = 0;
        if (scanf("%d %d", &S, &M) != 2 || S < 1 || M < 1) return 2;
        std::vector<int> nser(S), series(M);
        if (!rd(nser) || !rd(series)) return 2;
        const MfilterPlan pl = mfilter_plan(series.data(), M, nser.data());
        put1("W", pl.W);
        put1("tile_total", (long long)pl.tile_total);
        put1("nmax", pl.nmax);
        put("offs", pl.offs);
        put("order", pl.order);
        put("tint", pl.tint);
        put("tlong", pl.tlong);
        return 0;
    }
    if (!strcmp(mode, "predict")) {
        int G = 0, S = 0, M = 0;
        if (scanf("%d %d %d", &G, &S, &M) != 3 || S < 1 || M < 1) return 2;
        std::vector<int> nser(S), series(M);
        std::vector<long> toff((size_t)M + 1);
        if (!rd(nser) || !rd(series) || !rd(toff)) return 2;
        SeriesBuckets b;
        const MpredictPlan pl = mpredict_plan(G, series.data(), M, S, nser.data(), toff.data(), b);
        put1("W", pl.W);
        put1("T", pl.T);
        put1("E", pl.E);
        put("tint", pl.tint);
        put("tlong", pl.tlong);
        return 0;
    }
    if (!strcmp(mode, "smooth")) {
        int G = 0, S = 0, M = 0;
        long forced = 0;
        if (scanf("%d %d %d %ld", &G, &S, &M, &forced) != 4 || S < 1 || M < 1) return 2;
        std::vector<int> nser(S), series(M);
        if (!rd(nser)) return 2;
        std::vector<long> hoff((size_t)S + 1, 0), toff((size_t)M + 1);
        for (int s = 0; s < S; s++) hoff[s + 1] = hoff[s] + nser[s];
        std::vector<double> t((size_t)hoff[S]);
        if (!rd(t) || !rd(series) || !rd(toff)) return 2;
        std::vector<double> tout((size_t)toff[M]);
        if (!rd(tout)) return 2;
        const MsmoothPlan pl = msmooth_plan(G, series.data(), M, tout.data(), toff.data(), t.data(), hoff.data(), nser.data(), forced);
        put1("E", pl.E);
        put1("W", pl.W);
        put1("J", pl.J);
        put1("pts_max", (long long)pl.pts_max);
        put("chunk0", pl.chunk0);
        put("tint", pl.tint);
        put("tlong", pl.tlong);
        printf("grids");
        for (double v : pl.grids) printf(" %.17g", v);
        printf("\n");
        return 0;
    }
    fprintf(stderr, "plan_main: unknown mode %s\n", mode);
    return 1;
}
