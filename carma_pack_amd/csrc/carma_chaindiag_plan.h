// carma_chaindiag_plan.h -- the host-only decisions of carma_chain_diag (carma_chaindiag.hip): the constants of the estimator, the
// shape of the kernel's LDS arena, which levels of the halving stay in LDS, and the layout of the call's one device block.
// Standard C++ only (no HIP): tests/chaindiag/plan_main.cpp exercises it on its own.
#pragma once
#include <cstddef>

#ifdef __HIPCC__
#define CD_HD __host__ __device__
#else
#define CD_HD
#endif

namespace carma {

constexpr int CD_MAXLAG = 10, CD_WINMULT = 5, CD_MINFAC = 5;   // Goodman's acor
constexpr int CD_DMAX = 16;                 // widest column count of one call: 3 + p + q at PMAX = 7, q = 6
constexpr int CD_T = 512;                   // threads of k_chain_diag
constexpr int CD_CAP = 5376;                // doubles of its LDS arena (42 KiB): a tile with its halo, or a whole resident level
constexpr int CD_NQ = 16;                   // quantities one block reduction carries (11 lag sums, sums and squares of the halves)

enum { CD_OK = 0, CD_SHORT = 1, CD_CONSTANT = 2, CD_NONFINITE = 3 };

// columns padded to a power of two: thread = row lane * dp + column
CD_HD static inline int cd_dpad(int d)
{
    int dp = 1;
    while (dp < d) dp <<= 1;
    return dp;
}
// a level of `rows` rows stays in LDS
CD_HD static inline bool cd_fits(long rows, int d) { return rows <= (long)(CD_CAP / d); }
// rows of a streamed tile, the MAXLAG rows of halo behind them not counted
CD_HD static inline int cd_tile_rows(int d) { return CD_CAP / d - CD_MAXLAG; }
// rows per block of the workspace that holds the halved levels which do not fit LDS: level 1 has L / 2 rows and every later one is
// written over it in place; none when level 1 fits already
static inline long cd_ws_rows(long L, int d) { return cd_fits(L / 2, d) ? 0 : L / 2; }
// levels a column can go through before L < MINFAC * MAXLAG ends it (level 0 included; 1 for L < 50)
static inline int cd_max_levels(long L)
{
    int k = 1;
    while (L >= CD_MINFAC * CD_MAXLAG) {
        L /= 2;
        k++;
    }
    return k;
}
// first level that is resident in LDS
static inline int cd_first_resident(long L, int d)
{
    int k = 0;
    while (!cd_fits(L, d)) {
        L /= 2;
        k++;
    }
    return k;
}

// The one device block of a call: [x][workspace][tau, mean, sigma: nb * d doubles each][rhat: G * d][half means, half sums of
// squares: nb * 2 * d each][status: nb * d ints]; everything from `out` to the end comes back in one copy.
struct ChainDiagPlan {
    long nb = 0;                            // chain blocks: G * R
    long ws_rows = 0;
    size_t o_x = 0, o_ws = 0, o_out = 0, o_tau = 0, o_mean = 0, o_sigma = 0, o_rhat = 0, o_hmean = 0, o_hm2 = 0, o_status = 0, bytes = 0;
    size_t out_bytes() const { return bytes - o_out; }
};

static inline size_t cd_round(size_t n) { return (n + 255) & ~(size_t)255; }

// false: the sizes do not fit size_t / the grid (more than 2^31 - 1 blocks, or more than 2^62 bytes)
static inline bool cd_plan(long G, int R, long L, int d, ChainDiagPlan* p)
{
    if (G < 1 || R < 1 || L < 1 || d < 1 || d > CD_DMAX) return false;
    const long double nbl = (long double)G * R;
    if (nbl > 2147483647.0L) return false;
    if (nbl * (long double)L * d * 1.5L * 8.0L + nbl * d * 64.0L > 4.0e18L) return false;
    p->nb = G * (long)R;
    p->ws_rows = cd_ws_rows(L, d);
    const size_t nbd = (size_t)p->nb * d;
    p->o_x = 0;
    p->o_ws = p->o_x + cd_round(sizeof(double) * (size_t)p->nb * (size_t)L * d);
    p->o_out = p->o_ws + cd_round(sizeof(double) * (size_t)p->nb * (size_t)p->ws_rows * d);
    p->o_tau = p->o_out;
    p->o_mean = p->o_tau + cd_round(sizeof(double) * nbd);
    p->o_sigma = p->o_mean + cd_round(sizeof(double) * nbd);
    p->o_rhat = p->o_sigma + cd_round(sizeof(double) * nbd);
    p->o_hmean = p->o_rhat + cd_round(sizeof(double) * (size_t)G * d);
    p->o_hm2 = p->o_hmean + cd_round(sizeof(double) * 2 * nbd);
    p->o_status = p->o_hm2 + cd_round(sizeof(double) * 2 * nbd);
    p->bytes = p->o_status + cd_round(sizeof(int) * nbd);
    return true;
}

}  // namespace carma
