// carma_pt_sched.h -- what the parallel-tempering samplers decide on the host, host C++ only: no HIP, nothing but the standard
// library and carma_types.h.  One copy for carma_pt_* (carma_pt_host.hip: one series) and the handle-based lane samplers
// (carma_pt_front.hip: carma_mpt_* on many series, carma_bands_pt_*, carma_bandset_pt_*):
// the default ladder, the initial proposal factor, the length of the next launch, the starting-value draws and the search for
// finite starting values.  tests/ptsched/ compiles it with a plain C++ compiler.
#ifndef CARMA_PT_SCHED_H
#define CARMA_PT_SCHED_H

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <random>
#include <vector>

#include "carma_types.h"

namespace carma {

inline double pop_var(const double* y, long n)
{
    // src/carmcmc.cpp:85-88
    double sum = 0, sq = 0;
    for (long i = 0; i < n; i++) {
        sum += y[i];
        sq += y[i] * y[i];
    }
    const double mean = sum / (size_t)n;
    return sq / (size_t)n - mean * mean;
}

inline double sample_var(const double* y, int n)   // arma::var
{
    double mean = 0;
    for (int i = 0; i < n; i++) mean += y[i];
    mean /= (size_t)n;
    double s = 0;
    for (int i = 0; i < n; i++) s += (y[i] - mean) * (y[i] - mean);
    return s / ((size_t)n - 1);
}

// The ladder of T temperatures: the caller's, or src/carmcmc.cpp:92-95: exp(linspace(0, ln 100, nwalkers))
inline void default_ladder(int T, const double* temperatures, std::vector<double>& out)
{
    out.resize(T);
    for (int i = 0; i < T; i++) {
        if (temperatures)
            out[i] = temperatures[i];
        else
            out[i] = (T == 1) ? 1.0 : std::exp(std::log(100.0) * (double)i / (double)(T - 1));
    }
}

// Initial proposal factor R0[d][d] of a sampler on a series of n data with population variance var (src/carmcmc.cpp:132-136 /
// :50-54, covariance diag(1e-4), [0,0] = 2 var^2 / n, [2,2] = var / n): diag 0.01, [0,0] = sqrt(2 var^2 / n), [2,2] = sqrt(var / n)
inline void initial_factor(double var, long n, int d, double* R0)
{
    std::fill(R0, R0 + (size_t)d * d, 0.0);
    for (int i = 0; i < d; i++) R0[(size_t)i * d + i] = 0.01;
    R0[0] = std::sqrt(2.0 * var * var / n);
    R0[(size_t)2 * d + 2] = std::sqrt(var / n);
}

// Iterations of the next launch when `left` remain and a launch takes chunk0.  thin > 0 (a sample every thin iterations): whole
// thinning intervals per launch, so that a launch's samples are its iterations / thin.
inline long pt_next_chunk(long left, long chunk0, int thin)
{
    long ch = std::min(left, chunk0);
    if (thin > 0) {
        ch = std::max<long>(thin, (ch / thin) * thin);
        ch = std::min(ch, left);
    }
    return ch;
}

// One draw from the reference's starting-value distribution for the series (t, y)[n] (sorted, distinct times) with prior pr.
inline void draw_start(const double* t, const double* y, int n, const Prior& pr, int p, int q, std::mt19937_64& rng, double* theta)
{
    std::normal_distribution<double> norm(0.0, 1.0);
    std::uniform_real_distribution<double> unif(0.0, 1.0);
    auto scaled_inv_chisq = [&](int dof, double ssqr) {       // src/random.cpp:180-186
        std::chi_squared_distribution<double> chi(dof);
        return ssqr / chi(rng) * (double)dof;
    };
    double ymean = 0;
    for (int i = 0; i < n; i++) ymean += y[i];
    ymean /= n;
    const double yvar = scaled_inv_chisq(n - 1, sample_var(y, n));
    const double mu = ymean + std::sqrt(yvar) / n * norm(rng);
    double scale = scaled_inv_chisq((int)pr.measerr_dof, 1.0);
    scale = std::max(std::min(scale, 1.99), 0.51);
    theta[0] = std::sqrt(yvar);
    theta[1] = scale;
    theta[2] = mu;
    if (p == 1) {
        // CAR1::StartingValue (src/carpack.cpp:38-81)
        std::vector<double> dt(n - 1);
        for (int i = 1; i < n; i++) dt[i - 1] = t[i] - t[i - 1];
        std::sort(dt.begin(), dt.end());
        const double med = (dt.size() % 2) ? dt[dt.size() / 2] : 0.5 * (dt[dt.size() / 2 - 1] + dt[dt.size() / 2]);
        double lw = -1.0 * std::log(med * (1.0 + 49.0 * unif(rng)));
        lw = std::min(lw, pr.max_freq);     // sic (carpack.cpp:56)
        theta[3] = lw;
        return;
    }
    // CARp::StartingAR (src/carpack.cpp:268-311)
    const double min_freq = pr.min_freq, max_freq = pr.max_freq;
    const int nc = (p + 1) / 2;
    std::vector<double> cent(nc), width(nc);
    for (int i = 0; i < nc; i++) cent[i] = std::exp(std::log(max_freq / min_freq) * unif(rng) + std::log(min_freq));
    std::sort(cent.begin(), cent.end(), std::greater<double>());
    for (int i = 0; i < nc; i++) width[i] = std::exp(std::log(max_freq / min_freq) * unif(rng) + std::log(min_freq));
    if (p % 2 == 1) {
        cent[p / 2] = 0.0;
        const double lo = std::log(min_freq), hi = std::log(cent[p / 2 - 1]);
        width[p / 2] = std::exp(lo + (hi - lo) * unif(rng));
    }
    for (int i = 0; i < p / 2; i++) {
        const double re = -2.0 * M_PI * width[i], im = 2.0 * M_PI * cent[i];
        theta[3 + 2 * i] = std::log(re * re + im * im);
        theta[3 + 2 * i + 1] = std::log(-2.0 * re);
    }
    if (p % 2 == 1) theta[3 + p - 1] = std::log(2.0 * M_PI * width[p / 2]);
    // CARMA::StartingMA (src/carpack.cpp:515-519)
    for (int i = 0; i < q; i++) theta[3 + p + i] = std::fabs(norm(rng));
}

// The generator of a chain's starting-value draws: keyed by (seed, the chain's GLOBAL slot, attempt)
inline std::mt19937_64 start_rng(uint64_t seed, uint64_t gslot, int round)
{
    uint64_t z = seed * 0x9E3779B97F4A7C15ull + 0x1234567ull;
    z ^= (gslot + 1) * 0xBF58476D1CE4E5B9ull;
    z ^= ((uint64_t)round + 1) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return std::mt19937_64(z * 0xD6E8FEB86659FD93ull + 0x2545F4914F6CDD1Dull);
}

// Finite starting values for the chains not yet done[k]: up to START_ROUNDS rounds, each of which draws a candidate for every chain
// still pending and evaluates them together; a chain keeps the first candidate whose log-posterior is finite (theta[k][d], lp[k],
// done[k] = 1).  Chains that come in done are left alone; chains still pending after the last round stay done[k] = 0 for the
// caller to report.
//   draw(k, round, out[d])           the candidate of chain k in this round
//   evaluate(cand, idx, m, out)      out[i] = log-posterior of cand[i][d], the candidate of chain idx[i], i < m; returns 0, or an
//                                    error code that ends the search and is returned as it is
constexpr int START_ROUNDS = 4000;

template <class Draw, class Evaluate>
int find_starts(size_t nchain, int d, double* theta, double* lp, char* done, Draw&& draw, Evaluate&& evaluate)
{
    std::vector<size_t> todo;
    std::vector<double> cand, out;
    for (int round = 0; round < START_ROUNDS; round++) {
        todo.clear();
        for (size_t k = 0; k < nchain; k++)
            if (!done[k]) todo.push_back(k);
        if (todo.empty()) break;
        cand.resize(todo.size() * d);
        out.resize(todo.size());
        for (size_t i = 0; i < todo.size(); i++) draw(todo[i], round, &cand[i * d]);
        const int rc = evaluate(cand.data(), todo.data(), todo.size(), out.data());
        if (rc != 0) return rc;
        for (size_t i = 0; i < todo.size(); i++) {
            if (std::isfinite(out[i])) {
                std::memcpy(&theta[todo[i] * d], &cand[i * d], sizeof(double) * d);
                lp[todo[i]] = out[i];
                done[todo[i]] = 1;
            }
        }
    }
    return 0;
}

}  // namespace carma

#endif
