// carma_mband_set_plan.h -- the host-only decisions of the calls on a SET of multi-band objects (carma_mband_set.hip): the layout
// and the argument checks of carma_bandset_create, the per-start boxes of carma_bandset_mle_batched and the evaluator it hands to
// mle_loop.  No HIP: the tests compile it stand-alone (tests/mbandset/mbandset_host.cpp).
//
// A set is S objects that share K, p and q, so dx is one number: object s is bands [s K, (s + 1) K) of one offset table
// [S K + 1] over the caller's arrays.  An object that lacks a band belongs to another set.  The launch plan of the set's
// log-density is mlogdens_plan_count / mlogdens_plan_fill of carma_mseries_plan.h as they stand, with nser = the objects' N and
// repdt all zero: waves of 64 evaluations of ONE object, the longest object first, ties in object order.
#ifndef CARMA_MBAND_SET_PLAN_H
#define CARMA_MBAND_SET_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "carma_mband_plan.h"
#include "carma_mseries_plan.h"

namespace carma {

// offsets of object s rebased to its first datum: [K + 1], as carma_bands_create takes them
inline void mbandset_object_offsets(const long* offsets, int s, int K, long* loc)
{
    const long base = offsets[(size_t)s * K];
    for (int b = 0; b <= K; b++) loc[b] = offsets[(size_t)s * K + b] - base;
}

// What carma_bandset_create refuses, as a message ("" = fine): mband_check_create of every object, the object named.
// offsets = [S K + 1]; lag_lo / lag_hi = [S][K - 1].
inline std::string mbandset_check_create(const double* time, const double* y, const double* yerr, const long* offsets, int S, int K,
                                         int p, int q, const double* lag_lo, const double* lag_hi)
{
    char buf[384];
    if (!time || !y || !yerr || !offsets) return "need non-null time, y, yerr and offsets";
    if (S < 1) {
        snprintf(buf, sizeof(buf), "need nobjects >= 1 (got %d)", S);
        return buf;
    }
    if (K < 1 || K > MBAND_PLAN_KMAX) {
        snprintf(buf, sizeof(buf), "need 1 <= nbands <= %d (got %d)", MBAND_PLAN_KMAX, K);
        return buf;
    }
    if (offsets[0] != 0) return "offsets[0] must be 0";
    long loc[MBAND_PLAN_KMAX + 1];
    for (int s = 0; s < S; s++) {
        const long base = offsets[(size_t)s * K];
        mbandset_object_offsets(offsets, s, K, loc);
        const std::string bad = mband_check_create(time + base, y + base, yerr + base, loc, K, p, q,
                                                   lag_lo ? lag_lo + (size_t)s * (K - 1) : nullptr,
                                                   lag_hi ? lag_hi + (size_t)s * (K - 1) : nullptr);
        if (!bad.empty()) {
            snprintf(buf, sizeof(buf), "object %d: %s", s, bad.c_str());
            return buf;
        }
    }
    return "";
}

// The boxes of carma_bandset_mle_batched: lo / hi = [B][dx] (no NULLs, +-inf = unbounded); the lag entries of start i are cut to
// the lag box of object[i] (lagbox = [S][K - 1][2]).  -1, or the first start of which nothing is left (band: which lag); with
// fixed lags the lag entries are not read and nothing is refused.
inline long mbandset_cut_boxes(double* lo, double* hi, const int* object, int B, int d, int K, const double* lagbox, bool fixed,
                               int* band)
{
    const int dx = mband_dim(d, K);
    for (long i = 0; i < B; i++)
        for (int b = 1; b < K; b++) {
            const size_t j = (size_t)i * dx + d + 3 * (b - 1);
            const double* box = lagbox + ((size_t)object[i] * (K - 1) + (b - 1)) * 2;
            lo[j] = std::max(lo[j], box[0]);
            hi[j] = std::min(hi[j], box[1]);
            if (!fixed && lo[j] > hi[j]) {
                if (band) *band = b;
                return i;
            }
        }
    return -1;
}

// The set's log-density with the objects of the points in flight bound to it: what EvalBands calls
template <class Dens>
struct SetDens {
    Dens dens;                        // dens(thx [npts][dx], object [npts], npts, out [npts]) -> CARMA_OK or an error code
    const std::vector<int>* obj;
    int operator()(const double* thx, int npts, double* out) const { return dens(thx, obj->data(), npts, out); }
};

// The evaluator of carma_bandset_mle_batched: EvalBands (its fixed lags, its reduce / expand) with every point on the object of
// the start it belongs to -- one call of the set's log-density per optimiser step, for all objects.
template <class Dens>
struct EvalBandsSet : EvalBands<SetDens<Dens>> {
    using Base = EvalBands<SetDens<Dens>>;
    const int* object;                // [B] object of each start
    std::vector<int> obj;
    EvalBandsSet(Dens dens, int d, int K, const int* object_, const double* fixed_lag)
        : Base{SetDens<Dens>{dens, nullptr}, d, K, fixed_lag, {}, {}}, object(object_)
    {
        this->dens.obj = &obj;
    }
    EvalBandsSet(const EvalBandsSet&) = delete;
    EvalBandsSet& operator=(const EvalBandsSet&) = delete;
    int operator()(const std::vector<double>& pts, const std::vector<int>& owner, int npts)
    {
        obj.resize((size_t)npts);
        for (int i = 0; i < npts; i++) obj[i] = object[owner[i]];
        return Base::operator()(pts, owner, npts);
    }
};

// carma_bandset_mle_batched behind its argument checks: B starts x0 = [B][dx], start i on object[i] in its own box lo / hi =
// [B][dx] (mbandset_cut_boxes done).  With fixed_lag = [B][K - 1] the lag entries of x0, lo and hi are not read and x_out
// carries the fixed lags unchanged, as mband_mle_run.
template <class Dens>
int mbandset_mle_run(Dens dens, int d, int K, const double* x0, const int* object, int B, const double* lo, const double* hi,
                     const double* fixed_lag, int maxiter, int mem, double ftol, double gtol, double fd_step, double* x_out,
                     double* fun_out, int* nit, int* nfev, int* status)
{
    EvalBandsSet<Dens> fun(dens, d, K, object, fixed_lag);
    const int dx = mband_dim(d, K);
    if (!fixed_lag)
        return mle_loop(fun, dx, x0, B, lo, hi, (size_t)dx, maxiter, mem, ftol, gtol, fd_step, x_out, fun_out, nit, nfev, status);
    const int dr = mband_free_dim(d, K, true);
    std::vector<double> xr((size_t)B * dr), lor((size_t)B * dr), hir((size_t)B * dr), xo((size_t)B * dr);
    for (int i = 0; i < B; i++) {
        fun.reduce(x0 + (size_t)i * dx, &xr[(size_t)i * dr]);
        fun.reduce(lo + (size_t)i * dx, &lor[(size_t)i * dr]);
        fun.reduce(hi + (size_t)i * dx, &hir[(size_t)i * dr]);
    }
    const int rc = mle_loop(fun, dr, xr.data(), B, lor.data(), hir.data(), (size_t)dr, maxiter, mem, ftol, gtol, fd_step, xo.data(),
                            fun_out, nit, nfev, status);
    if (rc != CARMA_OK) return rc;
    for (int i = 0; i < B; i++) fun.expand(&xo[(size_t)i * dr], fixed_lag + (size_t)i * (K - 1), x_out + (size_t)i * dx);
    return CARMA_OK;
}

}  // namespace carma

#endif
