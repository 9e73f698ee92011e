// carma_prep.h -- what every create call does to the caller's data before anything goes to the device: sort and de-duplicate a
// series, the prior bounds and their default, the record buffer of a multi-band object.  Host C++ only, no HIP: the contexts
// (carma_capi.hip, carma_mseries.hip, carma_mband.hip, carma_mband_set.hip) and the test harnesses compile the same text.
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>
#include <numeric>
#include <vector>

#include "carma_types.h"

namespace carma {

// KalmanFilter::init (src/include/kfilter.hpp:43-76): sort by time when any dt < 0, then keep
// sample 0 and every sample whose dt to its predecessor in the sorted series is non-zero.
inline void sort_dedup(std::vector<double>& t, std::vector<double>& y, std::vector<double>& e)
{
    const size_t n = t.size();
    bool need_sort = false;
    for (size_t i = 1; i < n; i++) need_sort |= (t[i] - t[i - 1] < 0);
    if (need_sort) {
        std::vector<size_t> idx(n);
        std::iota(idx.begin(), idx.end(), 0);
        std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return t[a] < t[b]; });
        std::vector<double> t2(n), y2(n), e2(n);
        for (size_t i = 0; i < n; i++) {
            t2[i] = t[idx[i]];
            y2[i] = y[idx[i]];
            e2[i] = e[idx[i]];
        }
        t.swap(t2);
        y.swap(y2);
        e.swap(e2);
    }
    std::vector<char> keep(n, 1);
    bool dup = false;
    for (size_t i = 1; i < n; i++) {
        if (t[i] - t[i - 1] == 0) {
            keep[i] = 0;
            dup = true;
        }
    }
    if (dup) {
        size_t m = 0;
        for (size_t i = 0; i < n; i++) {
            if (keep[i]) {
                t[m] = t[i];
                y[m] = y[i];
                e[m] = e[i];
                m++;
            }
        }
        t.resize(m);
        y.resize(m);
        e.resize(m);
    }
}

// SetPrior (src/include/carpack.hpp:201-207) on a sorted, deduplicated series
inline void set_prior_bounds(Prior& pr, const double* t, long n, double max_stdev)
{
    pr.max_stdev = max_stdev;
    double dtmin = std::numeric_limits<double>::infinity();
    for (long i = 1; i < n; i++) dtmin = std::min(dtmin, t[i] - t[i - 1]);
    pr.max_freq = 1.0 / dtmin;
    pr.min_freq = 1.0 / (*std::max_element(t, t + n) - *std::min_element(t, t + n));
}

// The max_stdev of a context that is given none: 10 sqrt(var(y, ddof=1)) of the series as given (Context's default); 0 for n < 2
inline double default_max_stdev(const double* y, long n)
{
    if (n < 2) return 0.0;
    double mean = 0.0, ss = 0.0;
    for (long k = 0; k < n; k++) mean += y[k];
    mean /= (double)n;
    for (long k = 0; k < n; k++) ss += (y[k] - mean) * (y[k] - mean);
    return 10.0 * std::sqrt(ss / (double)(n - 1));
}

// what the *_get_prior calls hand out
inline void prior_out3(const Prior& pr, double* out3)
{
    out3[0] = pr.max_stdev;
    out3[1] = pr.max_freq;
    out3[2] = pr.min_freq;
}

// The record buffer of K bands (each sorted and de-duplicated already; n_b >= 1): {t - t0, y, yerr^2, 0} per datum, t0 the
// earliest time of all bands, and a sentinel {+inf, 0, 1, 0} behind every band.  boff = [K + 1].
inline void mband_pack(const std::vector<std::vector<double>>& t, const std::vector<std::vector<double>>& y,
                       const std::vector<std::vector<double>>& yerr, std::vector<double>& rec, std::vector<int>& boff)
{
    const int K = (int)t.size();
    double t0 = std::numeric_limits<double>::infinity();
    for (int b = 0; b < K; b++) t0 = std::min(t0, t[b][0]);
    boff.assign(K + 1, 0);
    rec.clear();
    for (int b = 0; b < K; b++) {
        for (size_t i = 0; i < t[b].size(); i++) {
            rec.push_back(t[b][i] - t0);
            rec.push_back(y[b][i]);
            rec.push_back(yerr[b][i] * yerr[b][i]);
            rec.push_back(0.0);
        }
        rec.push_back(std::numeric_limits<double>::infinity());
        rec.push_back(0.0);
        rec.push_back(1.0);
        rec.push_back(0.0);
        boff[b + 1] = (int)(rec.size() / 4);
    }
}

}  // namespace carma
