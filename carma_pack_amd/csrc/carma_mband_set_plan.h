// carma_mband_set_plan.h -- the host-only decisions of the calls on a SET of multi-band objects (carma_mband_set.hip): the layout,
// the argument checks and the preparation of carma_bandset_create and the evaluator carma_bandset_mle_batched hands to the
// optimiser's driver (mband_mle_drive; the per-start boxes are mband_cut_boxes, both of carma_mband_plan.h).  No HIP: the tests
// compile it stand-alone (tests/mbandset/mbandset_host.cpp).
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

// The prepared objects of a set side by side: object s as mband_prepare leaves it alone, its records from record off[s]
struct MbandSet {
    std::vector<int> n;               // [S][K] data per band after sort / dedup
    std::vector<int> N;               // [S] data per object: the trip count of its waves
    std::vector<int> boff;            // [S][K + 1] first record of a band, relative to the object's first
    std::vector<long> off;            // [S] first record of object s: the running record count
    std::vector<double> lagbox;       // [S][K - 1][2]
    std::vector<Prior> pr;            // [S]
    std::vector<double> t0;           // [S] the time origin of object s (MbandObject::t0): what its requested times are shifted by
    std::vector<std::vector<double>> ts, ys;   // [S][K] the bands' times and values after sort / dedup (MbandObject::ts / ys:
                                      // host only, what the set's sampler takes starting values, factors and boxes from)
    std::vector<double> rec;          // the records of all objects (an object keeps its own t0: the earliest time of ITS bands)
};

// mband_prepare of every object of a set that mbandset_check_create has passed (max_stdev = [S], or null: every object takes
// the default).  -1, or the first object of which fewer than 2 data are left.
inline int mbandset_prepare(const double* time, const double* y, const double* yerr, const long* offsets, int S, int K,
                            const double* lag_lo, const double* lag_hi, const double* max_stdev, MbandSet& m)
{
    m = MbandSet();
    MbandObject o;
    for (int s = 0; s < S; s++) {
        if (!mband_prepare(time, y, yerr, offsets + (size_t)s * K, K, lag_lo + (size_t)s * (K - 1), lag_hi + (size_t)s * (K - 1),
                           max_stdev ? max_stdev + s : nullptr, o))
            return s;
        m.off.push_back((long)(m.rec.size() / 4));
        m.rec.insert(m.rec.end(), o.rec.begin(), o.rec.end());
        m.n.insert(m.n.end(), o.n.begin(), o.n.end());
        m.N.push_back(o.N);
        m.boff.insert(m.boff.end(), o.boff.begin(), o.boff.end());
        m.lagbox.insert(m.lagbox.end(), o.lagbox.begin(), o.lagbox.end());
        m.pr.push_back(o.pr);
        m.t0.push_back(o.t0);
        for (int b = 0; b < K; b++) {
            m.ts.push_back(std::move(o.ts[b]));
            m.ys.push_back(std::move(o.ys[b]));
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

// mband_cut_boxes with a box per start: lo / hi = [B][dx], row i cut to the lag boxes of object[i]
inline long mbandset_cut_boxes(double* lo, double* hi, const int* object, int B, int d, int K, const double* lagbox, bool fixed, int* band)
{
    return mband_cut_boxes(lo, hi, object, B, d, K, lagbox, fixed, band);
}

// mband_mle_drive on a set: start i on object[i] in its own box lo / hi = [B][dx] (mbandset_cut_boxes done)
template <class Dens>
int mbandset_mle_run(Dens dens, int d, int K, const double* x0, const int* object, int B, const double* lo, const double* hi,
                     const double* fixed_lag, int maxiter, int mem, double ftol, double gtol, double fd_step, double* x_out,
                     double* fun_out, int* nit, int* nfev, int* status)
{
    EvalBandsSet<Dens> fun(dens, d, K, object, fixed_lag);
    return mband_mle_drive(fun, d, K, x0, B, lo, hi, B, fixed_lag, maxiter, mem, ftol, gtol, fd_step, x_out, fun_out, nit, nfev, status);
}

}  // namespace carma

#endif
