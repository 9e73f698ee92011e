// Stand-alone checks of carma_chaindiag_plan.h, the host-only level / workspace planner of carma_chain_diag: plain C++, no HIP.
//   plan_main <group>     group = shapes | levels | layout | limits; exits at the first failed check and names it
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "carma_chaindiag_plan.h"

using namespace carma;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static const long LENGTHS[] = {1, 2, 49, 50, 51, 99, 100, 101, 257, 335, 336, 337, 672, 673, 1023, 4099, 5376, 5377, 10752, 10753,
                               20000, 40000, 50000, 1000003, 2147483647L, 4294967311L};

static void shapes()
{
    CHECK(cd_dpad(1) == 1 && cd_dpad(2) == 2 && cd_dpad(3) == 4 && cd_dpad(4) == 4 && cd_dpad(5) == 8 && cd_dpad(11) == 16 &&
          cd_dpad(16) == 16);
    for (int d = 1; d <= CD_DMAX; d++) {
        CHECK(CD_T % cd_dpad(d) == 0 && cd_dpad(d) <= 64);                    // whole row lanes, a column's lanes inside a wave
        const int tr = cd_tile_rows(d);
        CHECK(tr >= 2 * CD_MAXLAG);
        CHECK((long)(tr + CD_MAXLAG) * d <= CD_CAP);                          // tile and halo fit the arena
        CHECK(cd_fits(CD_CAP / d, d) && !cd_fits(CD_CAP / d + 1, d));
        CHECK((long)(CD_CAP / d) * d <= CD_CAP);
    }
    CHECK(CD_NQ >= CD_MAXLAG + 3 && CD_NQ * CD_DMAX <= CD_T);
}

static void levels()
{
    for (long L : LENGTHS)
        for (int d = 1; d <= CD_DMAX; d++) {
            const long ws = cd_ws_rows(L, d);
            CHECK(ws == 0 || ws == L / 2);
            CHECK((ws == 0) == cd_fits(L / 2, d));
            // the walk the kernel makes: level k has L >> k rows; a level that does not fit is streamed (k = 0: from the input,
            // k >= 1: from the workspace), and once a level fits every later one does
            long rows = L;
            int k = 0, first = -1, nlev = 0;
            bool resident_seen = false;
            for (;; k++) {
                const bool fits = cd_fits(rows, d);
                if (fits && first < 0) first = k;
                if (resident_seen) CHECK(fits);
                resident_seen = resident_seen || fits;
                if (!fits && k >= 1) CHECK(rows <= ws);
                CHECK(rows == (L >> k));
                nlev++;
                if (rows < CD_MINFAC * CD_MAXLAG) break;
                rows /= 2;
            }
            CHECK(nlev == cd_max_levels(L));
            if (first >= 0) CHECK(first == cd_first_resident(L, d));
            else CHECK(cd_first_resident(L, d) >= nlev);
        }
}

static void layout()
{
    const long Gs[] = {1, 5, 64, 1024};
    const int Rs[] = {1, 3, 4};
    for (long G : Gs)
        for (int R : Rs)
            for (long L : {1L, 49L, 4099L, 20000L, 50000L})
                for (int d : {1, 4, 11, 16}) {
                    ChainDiagPlan p;
                    CHECK(cd_plan(G, R, L, d, &p));
                    const size_t nb = (size_t)G * R, nbd = nb * d;
                    CHECK(p.nb == (long)nb && p.ws_rows == cd_ws_rows(L, d));
                    const size_t off[] = {p.o_x, p.o_ws, p.o_out, p.o_mean, p.o_sigma, p.o_rhat, p.o_hmean, p.o_hm2, p.o_status, p.bytes};
                    const size_t need[] = {8 * nb * (size_t)L * d, 8 * nb * (size_t)p.ws_rows * d, 8 * nbd, 8 * nbd, 8 * nbd,
                                           8 * (size_t)G * d, 16 * nbd, 16 * nbd, 4 * nbd};
                    CHECK(p.o_x == 0 && p.o_tau == p.o_out);
                    for (int i = 0; i < 9; i++) {
                        CHECK(off[i] % 256 == 0);
                        CHECK(off[i + 1] >= off[i] + need[i]);                // regions in order, none overlapping
                        CHECK(off[i + 1] < off[i] + need[i] + 256);           // ... and no more padding than the alignment
                    }
                    CHECK(p.out_bytes() == p.bytes - p.o_out);
                    // what comes back in one copy can be walked without leaving a host buffer of out_bytes()
                    std::vector<unsigned char> out(p.out_bytes());
                    std::memset(out.data() + (p.o_status - p.o_out), 1, 4 * nbd);
                    std::memset(out.data() + (p.o_rhat - p.o_out), 2, 8 * (size_t)G * d);
                    CHECK(out[p.o_status - p.o_out + 4 * nbd - 1] == 1);
                }
    // the sizes the issue names exceed 2^31 elements and bytes
    ChainDiagPlan p;
    CHECK(cd_plan(1024, 1, 20000, 11, &p));
    CHECK(p.o_ws == 8ul * 1024 * 20000 * 11 && p.ws_rows == 10000 && p.bytes > (size_t)2700000000ul);
    CHECK(cd_plan(1, 1, 4294967311L, 1, &p) && p.o_ws >= 8ul * 4294967311ul);
}

static void limits()
{
    ChainDiagPlan p;
    CHECK(!cd_plan(0, 1, 1, 1, &p) && !cd_plan(1, 0, 1, 1, &p) && !cd_plan(1, 1, 0, 1, &p) && !cd_plan(1, 1, 1, 0, &p));
    CHECK(!cd_plan(-1, 1, 1, 1, &p) && !cd_plan(1, -1, 1, 1, &p) && !cd_plan(1, 1, -5, 1, &p));
    CHECK(!cd_plan(1, 1, 1, CD_DMAX + 1, &p) && cd_plan(1, 1, 1, CD_DMAX, &p));
    CHECK(cd_plan(2147483647L, 1, 1, 1, &p) && p.nb == 2147483647L);
    CHECK(!cd_plan(2147483648L, 1, 1, 1, &p));                               // more chain blocks than a grid holds
    CHECK(!cd_plan(1073741824L, 2, 1, 1, &p));
    CHECK(!cd_plan(9223372036854775807L, 2147483647, 9223372036854775807L, 16, &p));   // no overflow on the way to "no"
    CHECK(!cd_plan(1, 1, 9223372036854775807L, 16, &p));
}

int main(int argc, char** argv)
{
    const char* g = argc > 1 ? argv[1] : "";
    if (!std::strcmp(g, "shapes")) shapes();
    else if (!std::strcmp(g, "levels")) levels();
    else if (!std::strcmp(g, "layout")) layout();
    else if (!std::strcmp(g, "limits")) limits();
    else {
        std::printf("usage: plan_main shapes|levels|layout|limits\n");
        return 2;
    }
    std::printf("%s: all checks met\n", g);
    return 0;
}
