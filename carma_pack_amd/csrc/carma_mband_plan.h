// carma_mband_plan.h -- the host-only decisions of the multi-band calls, of one object (carma_mband.hip) and of a set
// (carma_mband_set.hip, carma_mband_set_plan.h): the argument checks of carma_bands_create, the preparation of an object
// (mband_prepare), and of the optimiser calls the boxes, the evaluator handed to mle_loop and the one driver around it.  No HIP:
// the tests instantiate the evaluator on an objective with a known answer (tests/mband/mband_mle_host.cpp) and prepare objects
// (tests/mbandset/mbandset_host.cpp).
#ifndef CARMA_MBAND_PLAN_H
#define CARMA_MBAND_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "carma_mle_loop.h"
#include "carma_prep.h"

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

// One multi-band object as the kernels and the host calls want it: every band prepared as carma_ctx_create prepares a series
struct MbandObject {
    int N = 0;                        // data in all: the trip count of the object's waves
    std::vector<int> n, boff;         // [K] data per band after sort / dedup, [K + 1] first record of a band (mband_pack)
    std::vector<double> lagbox;       // [K - 1][2]
    Prior pr{};
    double t0 = 0.0;                  // the time origin mband_pack subtracted: the earliest time of all bands
    std::vector<std::vector<double>> ts, ys;   // [K] the bands' times and values after sort / dedup
    std::vector<double> rec;          // the packed records, a sentinel behind each band (mband_pack)
};

// Fills o from arguments mband_check_create has passed: band b is [offsets[b], offsets[b + 1]) of time / y / yerr (offsets need
// not start at 0: an object of a set is prepared through the set's table).  max_stdev: null = 10 sqrt(var(y, ddof=1)) of band 0
// as given (BandsContext's default).  false: fewer than 2 data are left after the duplicate times of each band are dropped.
inline bool mband_prepare(const double* time, const double* y, const double* yerr, const long* offsets, int K, const double* lag_lo,
                          const double* lag_hi, const double* max_stdev, MbandObject& o)
{
    o = MbandObject();
    o.n.resize(K);
    o.ts.resize(K);
    o.ys.resize(K);
    std::vector<std::vector<double>> es(K);
    for (int b = 0; b < K; b++) {
        o.ts[b].assign(time + offsets[b], time + offsets[b + 1]);
        o.ys[b].assign(y + offsets[b], y + offsets[b + 1]);
        es[b].assign(yerr + offsets[b], yerr + offsets[b + 1]);
        sort_dedup(o.ts[b], o.ys[b], es[b]);
        o.n[b] = (int)o.ts[b].size();
        o.N += o.n[b];
    }
    if (o.N < 2) return false;
    o.pr.measerr_dof = 50.0;   // src/include/carpack.hpp:63
    set_prior_bounds(o.pr, o.ts[0].data(), o.n[0], max_stdev ? *max_stdev : default_max_stdev(y + offsets[0], offsets[1] - offsets[0]));
    for (int b = 0; b + 1 < K; b++) {
        o.lagbox.push_back(lag_lo[b]);
        o.lagbox.push_back(lag_hi[b]);
    }
    mband_pack(o.ts, o.ys, es, o.rec, o.boff);
    o.t0 = o.ts[0][0];                                        // (as mband_pack takes it: requested times get the same shift)
    for (int b = 1; b < K; b++) o.t0 = std::min(o.t0, o.ts[b][0]);
    return true;
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

// The optimiser behind the argument checks of carma_bands_mle_batched and carma_bandset_mle_batched: B starts x0 = [B][dx] in the
// boxes lo / hi = [nrows][dx] (no NULLs, +-inf = unbounded; the lag entries already cut, mband_cut_boxes) -- nrows = 1: one box
// for all starts, the stride mle_loop gets is 0; nrows = B: a box per start, the stride is the row.  fun: EvalBands, or what
// derives from it.  With fixed_lag = [B][K - 1] the lag entries of x0, lo and hi are not read, the run is on the dx - (K - 1)
// other variables and x_out carries the fixed lags unchanged.
template <class Eval>
int mband_mle_drive(Eval& fun, int d, int K, const double* x0, int B, const double* lo, const double* hi, int nrows,
                    const double* fixed_lag, int maxiter, int mem, double ftol, double gtol, double fd_step, double* x_out,
                    double* fun_out, int* nit, int* nfev, int* status)
{
    const int dx = mband_dim(d, K);
    const size_t rows = nrows > 1 ? 1 : 0;
    if (!fixed_lag)
        return mle_loop(fun, dx, x0, B, lo, hi, rows * dx, maxiter, mem, ftol, gtol, fd_step, x_out, fun_out, nit, nfev, status);
    const int dr = mband_free_dim(d, K, true);
    std::vector<double> xr((size_t)B * dr), lor((size_t)nrows * dr), hir((size_t)nrows * dr), xo((size_t)B * dr);
    for (int i = 0; i < B; i++) fun.reduce(x0 + (size_t)i * dx, &xr[(size_t)i * dr]);
    for (int r = 0; r < nrows; r++) {
        fun.reduce(lo + (size_t)r * dx, &lor[(size_t)r * dr]);
        fun.reduce(hi + (size_t)r * dx, &hir[(size_t)r * dr]);
    }
    const int rc = mle_loop(fun, dr, xr.data(), B, lor.data(), hir.data(), rows * dr, maxiter, mem, ftol, gtol, fd_step, xo.data(),
                            fun_out, nit, nfev, status);
    if (rc != CARMA_OK) return rc;
    for (int i = 0; i < B; i++) fun.expand(&xo[(size_t)i * dr], fixed_lag + (size_t)i * (K - 1), x_out + (size_t)i * dx);
    return CARMA_OK;
}

// ... of one object: dens(thx [npts][dx], npts, out [npts]), one box lo / hi = [dx]
template <class Dens>
int mband_mle_run(Dens dens, int d, int K, const double* x0, int B, const double* lo, const double* hi, const double* fixed_lag,
                  int maxiter, int mem, double ftol, double gtol, double fd_step, double* x_out, double* fun_out, int* nit, int* nfev,
                  int* status)
{
    EvalBands<Dens> fun{dens, d, K, fixed_lag, {}, {}};
    return mband_mle_drive(fun, d, K, x0, B, lo, hi, 1, fixed_lag, maxiter, mem, ftol, gtol, fd_step, x_out, fun_out, nit, nfev, status);
}

// The boxes of the two optimiser calls: lo / hi = [nrows][dx]; the lag entries of row i are cut to the lag box of object[i]
// (lagbox = [S][K - 1][2]; object = null: every row on object 0).  -1, or the first row of which nothing is left (band: which
// lag).  A lag never leaves its box, with or without the prior; with fixed lags the entries are not read and nothing is refused.
inline long mband_cut_boxes(double* lo, double* hi, const int* object, long nrows, int d, int K, const double* lagbox, bool fixed,
                            int* band)
{
    const int dx = mband_dim(d, K);
    for (long i = 0; i < nrows; i++)
        for (int b = 1; b < K; b++) {
            const size_t j = (size_t)i * dx + d + 3 * (b - 1);
            const double* box = lagbox + ((size_t)(object ? object[i] : 0) * (K - 1) + (b - 1)) * 2;
            lo[j] = std::max(lo[j], box[0]);
            hi[j] = std::min(hi[j], box[1]);
            if (!fixed && lo[j] > hi[j]) {
                if (band) *band = b;
                return i;
            }
        }
    return -1;
}

// fixed_lag = [B][K - 1] or null: -1, or the index of the first entry that is not finite (start i / (K - 1), band i % (K - 1) + 1)
inline long mband_fixed_lag_bad(const double* fixed_lag, int B, int K)
{
    if (fixed_lag)
        for (long i = 0; i < (long)B * (K - 1); i++)
            if (!std::isfinite(fixed_lag[i])) return i;
    return -1;
}

}  // namespace carma

#endif
