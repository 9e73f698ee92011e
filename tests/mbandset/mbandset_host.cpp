// mbandset_host.cpp -- TEST HARNESS ONLY: the host-only decisions of the calls on a set of multi-band objects
// (carma_pack_amd/csrc/carma_mband_set_plan.h) behind plain C entry points: the create checks, the per-start boxes, the lock-step
// optimiser on a log-density that calls back into the test -- so that tests/test_mbandset_cpu.py can run it on an objective whose
// answer is known and see the object of every point the evaluator hands on -- and the launch plan as carma_bandset_logdensity_batch
// asks for it (carma_mseries_plan.h, lengths = the objects' N, one cadence class) -- and the preparation of the objects, of the set
// as a whole and of one object alone, as bytes.  Host code, built by g++ (tests/mbandset_build.py).
#include "carma_mband_set_plan.h"

typedef int (*mbandset_dens_cb)(const double* thx, const int* object, int npts, double* out, void* user);

// carma_bandset_create's argument checks: 0 and an empty message, or CARMA_EINVAL and the message
extern "C" int mbandset_check_create_host(const double* time, const double* y, const double* yerr, const long* offsets, int S, int K,
                                          int p, int q, const double* lag_lo, const double* lag_hi, char* msg, int len)
{
    const std::string s = carma::mbandset_check_create(time, y, yerr, offsets, S, K, p, q, lag_lo, lag_hi);
    snprintf(msg, len, "%s", s.c_str());
    return s.empty() ? CARMA_OK : CARMA_EINVAL;
}

// mbandset_cut_boxes in place: -1, or the start nothing is left of (*band: which lag)
extern "C" long mbandset_cut_boxes_host(double* lo, double* hi, const int* object, int B, int d, int K, const double* lagbox, int fixed,
                                        int* band)
{
    return carma::mbandset_cut_boxes(lo, hi, object, B, d, K, lagbox, fixed != 0, band);
}

extern "C" int mbandset_mle_host(mbandset_dens_cb cb, void* user, int d, int K, const double* x0, const int* object, int B,
                                 const double* lo, const double* hi, const double* fixed_lag, int maxiter, int mem, double ftol,
                                 double gtol, double fd_step, double* x, double* fun, int* nit, int* nfev, int* status)
{
    if (!cb || d < 1 || K < 1 || K > CARMA_KBANDS_MAX || B < 0 || !object || !lo || !hi || mem < 1 || mem > 64 || maxiter < 0)
        return CARMA_EINVAL;
    auto dens = [cb, user](const double* thx, const int* obj, int npts, double* out) { return cb(thx, obj, npts, out, user); };
    return carma::mbandset_mle_run(dens, d, K, x0, object, B, lo, hi, fixed_lag, maxiter, mem, ftol, gtol, fd_step, x, fun, nit, nfev,
                                   status);
}

// The launch plan of B evaluations on S objects of N[s] data.  Returns the number of waves W (wave_obj = [W], eval_idx = [64 W],
// written when they hold cap_w waves), or -2 - i for the first object[i] out of range.
extern "C" long mbandset_plan_host(const int* object, int B, int S, const int* N, int* wave_obj, int* eval_idx, long cap_w)
{
    carma::MlogdensPlan pl;
    const std::vector<char> plain((size_t)S, 0);
    const long bad = carma::mlogdens_plan_count(object, B, S, N, plain.data(), pl);
    if (bad >= 0) return -2 - bad;
    if (pl.W <= cap_w) carma::mlogdens_plan_fill(pl, wave_obj, eval_idx);
    return pl.W;
}

// What the preparation leaves of object s, as bytes: its records, boff [K + 1], n [K], N, lagbox [K - 1][2] and the three prior
// numbers carma_*_get_prior hands out.  alone = 0: the slice of the set prepared as a whole (mbandset_prepare; max_stdev = [S] or
// null); alone = 1: the object prepared on its own, as carma_bands_create gets it -- its data rebased to offset 0, max_stdev[s]
// or null (mband_prepare).  Returns the byte count, -1 when fewer than 2 data are left, -2 when buf is too small.
extern "C" long mbandset_prepared_host(const double* time, const double* y, const double* yerr, const long* offsets, int S, int K,
                                       const double* lag_lo, const double* lag_hi, const double* max_stdev, int s, int alone,
                                       unsigned char* buf, long cap)
{
    std::vector<unsigned char> out;
    auto put = [&out](const void* p, size_t bytes) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        out.insert(out.end(), b, b + bytes);
    };
    double pr3[3];
    if (alone) {
        long loc[CARMA_KBANDS_MAX + 1];
        carma::mbandset_object_offsets(offsets, s, K, loc);
        const long base = offsets[(size_t)s * K];
        carma::MbandObject o;
        if (!carma::mband_prepare(time + base, y + base, yerr + base, loc, K, lag_lo + (size_t)s * (K - 1), lag_hi + (size_t)s * (K - 1),
                                  max_stdev ? max_stdev + s : nullptr, o))
            return -1;
        carma::prior_out3(o.pr, pr3);
        put(o.rec.data(), sizeof(double) * o.rec.size());
        put(o.boff.data(), sizeof(int) * o.boff.size());
        put(o.n.data(), sizeof(int) * o.n.size());
        put(&o.N, sizeof(int));
        put(o.lagbox.data(), sizeof(double) * o.lagbox.size());
    } else {
        carma::MbandSet m;
        if (carma::mbandset_prepare(time, y, yerr, offsets, S, K, lag_lo, lag_hi, max_stdev, m) >= 0) return -1;
        const size_t r0 = (size_t)m.off[s] * 4, r1 = s + 1 < S ? (size_t)m.off[s + 1] * 4 : m.rec.size();
        carma::prior_out3(m.pr[s], pr3);
        put(m.rec.data() + r0, sizeof(double) * (r1 - r0));
        put(m.boff.data() + (size_t)s * (K + 1), sizeof(int) * (K + 1));
        put(m.n.data() + (size_t)s * K, sizeof(int) * K);
        put(&m.N[s], sizeof(int));
        put(m.lagbox.data() + (size_t)s * 2 * (K - 1), sizeof(double) * 2 * (K - 1));
    }
    put(pr3, sizeof(pr3));
    if ((long)out.size() > cap) return -2;
    std::memcpy(buf, out.data(), out.size());
    return (long)out.size();
}
