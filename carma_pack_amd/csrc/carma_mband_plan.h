// carma_mband_plan.h -- the host-only decisions of the multi-band calls (carma_mband.hip): the argument checks of
// carma_bands_create and the evaluator that carma_bands_mle_batched hands to mle_loop.  No HIP: the tests instantiate the
// evaluator on an objective with a known answer (tests/mband/mband_mle_host.cpp).
#ifndef CARMA_MBAND_PLAN_H
#define CARMA_MBAND_PLAN_H

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "carma_mle_loop.h"

namespace carma {

constexpr int MBAND_PLAN_KMAX = CARMA_KBANDS_MAX;

// dx = d + 3 (K - 1): the CARMA part, then (lag_b, log a_b, mu_b) for b = 1 ... K - 1
inline int mband_dim(int d, int K) { return d + 3 * (K - 1); }
// variables the optimiser runs on: all of them, or all but the K - 1 lags
inline int mband_free_dim(int d, int K, bool fixed_lag) { return mband_dim(d, K) - (fixed_lag ? K - 1 : 0); }

// What carma_bands_create refuses, as a message ("" = fine).  offsets = [K + 1]; lag_lo / lag_hi = [K - 1].
inline std::string mband_check_create(const double* time, const double* y, const double* yerr, const long* offsets, int K, int p,
                                      int q, const double* lag_lo, const double* lag_hi)
{
    char buf[256];
    if (!time || !y || !yerr || !offsets) return "need non-null time, y, yerr and offsets";
    if (K < 1 || K > MBAND_PLAN_KMAX) {
        snprintf(buf, sizeof(buf), "need 1 <= nbands <= %d (got %d)", MBAND_PLAN_KMAX, K);
        return buf;
    }
    if (p < 1 || p > CARMA_PMAX || q < 0 || q >= p) {
        snprintf(buf, sizeof(buf), "need 1 <= p <= %d and q < p (got p=%d q=%d)", CARMA_PMAX, p, q);
        return buf;
    }
    if (offsets[0] != 0) return "offsets[0] must be 0";
    for (int b = 0; b < K; b++) {
        if (offsets[b + 1] <= offsets[b]) {
            snprintf(buf, sizeof(buf), "band %d is empty or offsets decrease (offsets[%d]=%ld, offsets[%d]=%ld)", b, b, offsets[b],
                     b + 1, offsets[b + 1]);
            return buf;
        }
    }
    if (offsets[K] < 2) return "need at least 2 data in all";
    if (offsets[K] > 0x3fffffffL) return "more data than an int can count";
    for (long i = 0; i < offsets[K]; i++)
        if (!std::isfinite(time[i]) || !std::isfinite(y[i]) || !std::isfinite(yerr[i])) {
            snprintf(buf, sizeof(buf), "datum %ld is not finite", i);
            return buf;
        }
    if (K > 1 && (!lag_lo || !lag_hi)) return "need lag_lo and lag_hi for nbands > 1";
    for (int b = 0; b + 1 < K; b++)
        if (!std::isfinite(lag_lo[b]) || !std::isfinite(lag_hi[b]) || lag_lo[b] > lag_hi[b]) {
            snprintf(buf, sizeof(buf), "lag box of band %d: need finite lag_lo <= lag_hi (got %g, %g)", b + 1, lag_lo[b], lag_hi[b]);
            return buf;
        }
    return "";
}

// The evaluator of carma_bands_mle_batched.  dens(thx [npts][dx], npts, out [npts]) computes the log-densities and returns CARMA_OK
// or an error code.  Without fixed lags the points ARE extended vectors.  With them (fixed_lag = [B][K - 1]) a point holds the
// dx - (K - 1) other variables -- the CARMA part, then (log a_b, mu_b) per band -- and the lags of the start it belongs to
// (owner) are put in: a lag is never a variable with an empty box, whose difference stencil would have no width.
template <class Dens>
struct EvalBands {
    static constexpr bool PER_START = true;
    Dens dens;
    int d, K;
    const double* fixed_lag;
    std::vector<double> out, full;
    int operator()(const std::vector<double>& pts, const std::vector<int>& owner, int npts)
    {
        out.resize((size_t)npts);
        if (npts == 0) return CARMA_OK;
        int rc;
        if (!fixed_lag) {
            rc = dens(pts.data(), npts, out.data());
        } else {
            const int dx = mband_dim(d, K), dr = mband_free_dim(d, K, true);
            full.resize((size_t)npts * dx);
            for (int i = 0; i < npts; i++) expand(&pts[(size_t)i * dr], fixed_lag + (size_t)owner[i] * (K - 1), &full[(size_t)i * dx]);
            rc = dens(full.data(), npts, out.data());
        }
        if (rc != CARMA_OK) return rc;
        for (int i = 0; i < npts; i++) {
            const double f = -out[i];
            out[i] = std::isfinite(f) ? f : BIG;
        }
        return CARMA_OK;
    }
    // reduced point + the lags of its start -> extended vector; and back
    void expand(const double* red, const double* lags, double* thx) const
    {
        for (int j = 0; j < d; j++) thx[j] = red[j];
        for (int b = 1; b < K; b++) {
            thx[d + 3 * (b - 1)] = lags[b - 1];
            thx[d + 3 * (b - 1) + 1] = red[d + 2 * (b - 1)];
            thx[d + 3 * (b - 1) + 2] = red[d + 2 * (b - 1) + 1];
        }
    }
    void reduce(const double* thx, double* red) const
    {
        for (int j = 0; j < d; j++) red[j] = thx[j];
        for (int b = 1; b < K; b++) {
            red[d + 2 * (b - 1)] = thx[d + 3 * (b - 1) + 1];
            red[d + 2 * (b - 1) + 1] = thx[d + 3 * (b - 1) + 2];
        }
    }
};

// carma_bands_mle_batched behind its argument checks: B starts x0 = [B][dx] in the box lo / hi = [dx] (no NULLs, +-inf =
// unbounded; the lag entries already cut to the lag boxes).  With fixed_lag the lag entries of x0, lo and hi are not read and
// x_out carries the fixed lags unchanged.
template <class Dens>
int mband_mle_run(Dens dens, int d, int K, const double* x0, int B, const double* lo, const double* hi, const double* fixed_lag,
                  int maxiter, int mem, double ftol, double gtol, double fd_step, double* x_out, double* fun_out, int* nit, int* nfev,
                  int* status)
{
    EvalBands<Dens> fun{dens, d, K, fixed_lag, {}, {}};
    const int dx = mband_dim(d, K);
    if (!fixed_lag)
        return mle_loop(fun, dx, x0, B, lo, hi, 0, maxiter, mem, ftol, gtol, fd_step, x_out, fun_out, nit, nfev, status);
    const int dr = mband_free_dim(d, K, true);
    std::vector<double> xr((size_t)B * dr), lor(dr), hir(dr), xo((size_t)B * dr);
    for (int i = 0; i < B; i++) fun.reduce(x0 + (size_t)i * dx, &xr[(size_t)i * dr]);
    fun.reduce(lo, lor.data());
    fun.reduce(hi, hir.data());
    const int rc = mle_loop(fun, dr, xr.data(), B, lor.data(), hir.data(), 0, maxiter, mem, ftol, gtol, fd_step, xo.data(), fun_out,
                            nit, nfev, status);
    if (rc != CARMA_OK) return rc;
    for (int i = 0; i < B; i++) fun.expand(&xo[(size_t)i * dr], fixed_lag + (size_t)i * (K - 1), x_out + (size_t)i * dx);
    return CARMA_OK;
}

}  // namespace carma

#endif
