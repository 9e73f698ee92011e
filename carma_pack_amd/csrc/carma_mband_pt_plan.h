// carma_mband_pt_plan.h -- what the sampler of a multi-band fit (carma_bands_pt_*, carma_mband_pt.hip) decides on the host: the
// argument checks of its entry points, the initial proposal factor of the extended vector, the starting draw of a chain and the
// default box of the band terms.  Host C++ only, no HIP runtime: tests/mbandpt/mband_pt_plan_host.cpp puts it behind a C interface for the CPU tests.
//
// The extended vector (carma_mband_plan.h): the CARMA part [d = 3 + p + q], then (lag_b, log a_b, mu_b) for b = 1 ... K - 1.
// The band box.  logpost is flat in log a_b and mu_b, and as log a_b -> -inf the likelihood tends to a positive constant (band b
// explained by its error bars alone): the posterior is improper, and a chain at T = 100 can walk off for good.  The SAMPLER
// therefore confines (log a_b, mu_b) to a box; outside it a chain's log-density is -inf.  The log-density calls know no such box.
#ifndef CARMA_MBAND_PT_PLAN_H
#define CARMA_MBAND_PT_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "carma_pt_sched.h"

namespace carma {

constexpr int MBAND_PT_DMAX = 37;          // RAM_DMAX_WIDE of carma_shape_plan.h: (7,6) in 8 bands
constexpr long long MBAND_PT_CHAINS_MAX = 0x7fffffffLL - 64;   // chain indices are ints in the launch arguments

// a band as the host keeps it: sorted, distinct times
struct BandView {
    const double* t;
    const double* y;
    int n;
};

// What carma_bands_pt_create refuses, as a message ("" = fine).  band_lo / band_hi = [K - 1][2] for (log a_b, mu_b), both or neither.
inline std::string mband_pt_check_create(int ntemps, int nreplicas, int adapt_iters, int dx, int K, int n0, const double* band_lo,
                                         const double* band_hi)
{
    char buf[256];
    if (nreplicas < 1 || adapt_iters < 0) return "bad argument (nreplicas < 1 or adapt_iters < 0)";
    if (ntemps < 1 || ntemps > 64) {
        snprintf(buf, sizeof(buf), "a ladder is 1 ... 64 temperatures, the lanes of a wave (got %d)", ntemps);
        return buf;
    }
    const long long nc = (long long)nreplicas * ntemps;
    if (nc > MBAND_PT_CHAINS_MAX) {
        snprintf(buf, sizeof(buf), "%d replicas x %d temperatures = %lld chains, more than one launch can index (%lld)", nreplicas,
                 ntemps, nc, MBAND_PT_CHAINS_MAX);
        return buf;
    }
    if (dx > MBAND_PT_DMAX) {
        snprintf(buf, sizeof(buf), "the extended vector has %d entries, the sampler's bookkeeping holds %d at most", dx, MBAND_PT_DMAX);
        return buf;
    }
    if (n0 < 2) return "band 0 needs at least 2 data (the starting values and the proposal scale come from it)";
    if ((band_lo == nullptr) != (band_hi == nullptr)) return "band_lo and band_hi come together (both null: no box)";
    if (band_lo)
        for (int i = 0; i < 2 * (K - 1); i++)
            if (!(band_lo[i] <= band_hi[i])) {               // (also a NaN)
                snprintf(buf, sizeof(buf), "band box of band %d, %s: need lo <= hi (got %g, %g)", i / 2 + 1, i % 2 ? "mu" : "log a",
                         band_lo[i], band_hi[i]);
                return buf;
            }
    return "";
}

inline double band_mean(const BandView& b)
{
    double s = 0;
    for (int i = 0; i < b.n; i++) s += b.y[i];
    return s / b.n;
}
inline double median_dt(const BandView& b)
{
    std::vector<double> dt((size_t)b.n - 1);
    for (int i = 1; i < b.n; i++) dt[i - 1] = b.t[i] - b.t[i - 1];
    std::sort(dt.begin(), dt.end());
    return (dt.size() % 2) ? dt[dt.size() / 2] : 0.5 * (dt[dt.size() / 2 - 1] + dt[dt.size() / 2]);
}

// Initial proposal factor R0[dx][dx] (upper triangular, diagonal here): the CARMA block as initial_factor gives it for band 0; per
// band the lag entry = the median time step of band 0, the log a entry = 0.01, the mu entry = sqrt(var y_b / n_b) (population
// variance, as the [2,2] entry of band 0), 0.01 where n_b < 2 or the band is constant.
inline void mband_pt_initial_factor(const BandView* bands, int K, int d, double* R0)
{
    const int dx = d + 3 * (K - 1);
    std::vector<double> Rc((size_t)d * d);
    initial_factor(pop_var(bands[0].y, bands[0].n), bands[0].n, d, Rc.data());
    std::fill(R0, R0 + (size_t)dx * dx, 0.0);
    for (int i = 0; i < d; i++)
        for (int j = 0; j < d; j++) R0[(size_t)i * dx + j] = Rc[(size_t)i * d + j];
    const double step = median_dt(bands[0]);
    for (int b = 1; b < K; b++) {
        const int c = d + 3 * (b - 1);
        double smu = bands[b].n >= 2 ? std::sqrt(pop_var(bands[b].y, bands[b].n) / bands[b].n) : 0.01;
        if (!(smu > 0.0) || !std::isfinite(smu)) smu = 0.01;
        R0[(size_t)c * dx + c] = step;
        R0[(size_t)(c + 1) * dx + c + 1] = 0.01;
        R0[(size_t)(c + 2) * dx + c + 2] = smu;
    }
}

// log a_b a chain starts from: log(std y_b / std y_0) (sample standard deviations), 0 where that is undefined
inline double mband_pt_start_log_a(const BandView* bands, int b)
{
    if (bands[b].n < 2 || bands[0].n < 2) return 0.0;
    const double v = std::log(std::sqrt(sample_var(bands[b].y, bands[b].n)) / std::sqrt(sample_var(bands[0].y, bands[0].n)));
    return std::isfinite(v) ? v : 0.0;
}

// The starting draw of chain `chain` in round `round`: the CARMA part from draw_start on band 0 with the chain's start_rng; then
// every lag uniform in its box from the same generator; log a_b and mu_b from the data (no draw).  lagbox = [K - 1][2].
inline void mband_pt_draw_start(const BandView* bands, int K, const Prior& pr, int p, int q, const double* lagbox, uint64_t seed,
                                uint64_t chain, int round, double* thx)
{
    const int d = 3 + p + q;
    std::mt19937_64 rng = start_rng(seed, chain, round);
    draw_start(bands[0].t, bands[0].y, bands[0].n, pr, p, q, rng, thx);
    std::uniform_real_distribution<double> unif(0.0, 1.0);
    for (int b = 1; b < K; b++) {
        const double lo = lagbox[2 * (b - 1)], hi = lagbox[2 * (b - 1) + 1];
        const int c = d + 3 * (b - 1);
        thx[c] = std::min(hi, std::max(lo, lo + (hi - lo) * unif(rng)));
        thx[c + 1] = mband_pt_start_log_a(bands, b);
        thx[c + 2] = band_mean(bands[b]);
    }
}

// The default box, lo / hi = [K - 1][2]: log a_b within +-log 1000 of its starting value, mu_b within [min y_b - span_b,
// max y_b + span_b], span_b = max y_b - min y_b (a band of one datum, or a constant one: span_b = max(1, |y_b|)).
inline void mband_pt_default_box(const BandView* bands, int K, double* lo, double* hi)
{
    for (int b = 1; b < K; b++) {
        const double la = mband_pt_start_log_a(bands, b);
        const double ymin = *std::min_element(bands[b].y, bands[b].y + bands[b].n);
        const double ymax = *std::max_element(bands[b].y, bands[b].y + bands[b].n);
        double span = ymax - ymin;
        if (!(span > 0.0)) span = std::max(1.0, std::fabs(ymax));
        lo[2 * (b - 1)] = la - std::log(1000.0);
        hi[2 * (b - 1)] = la + std::log(1000.0);
        lo[2 * (b - 1) + 1] = ymin - span;
        hi[2 * (b - 1) + 1] = ymax + span;
    }
}

// is (log a_b, mu_b) of every band of thx inside the box (null: no box)?  What the K1 of the sampler applies per chain.
inline bool mband_pt_in_box(const double* thx, int d, int K, const double* lo, const double* hi)
{
    if (!lo || !hi) return true;
    for (int i = 0; i < 2 * (K - 1); i++) {
        const double v = thx[d + 3 * (i / 2) + 1 + (i % 2)];
        if (!(v >= lo[i] && v <= hi[i])) return false;
    }
    return true;
}

// Iterations per chunk, as mpt_chunk_iters of carma_mpt.hip with the N data of all bands: an iteration's K1 runs ~0.45 us per
// datum; around a quarter of a second, at most 4096 iterations, are in flight at a time.
inline long mband_pt_chunk_iters(int N)
{
    const double est_us = std::max(1.0, 0.45 * N);
    return (long)std::max(1.0, std::min(4096.0, 250000.0 / est_us));
}

}  // namespace carma

#endif
