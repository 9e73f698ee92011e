// mband_mle_host.cpp -- TEST HARNESS ONLY: the multi-band optimiser entry behind its argument checks (mband_mle_run and the
// evaluator EvalBands of carma_pack_amd/csrc/carma_mband_plan.h, which put the fixed lags of a start into its points) on a
// log-density that calls back into the test, so that tests/test_mband_cpu.py can run it on an objective whose answer is known and
// see every extended vector the evaluator hands on.  Host code, built by g++ (tests/mband_build.py).
#include "carma_mband_plan.h"

typedef int (*mband_dens_cb)(const double* thx, int npts, double* out, void* user);

extern "C" int mband_mle_host(mband_dens_cb cb, void* user, int d, int K, const double* x0, int B, const double* lo, const double* hi,
                              const double* fixed_lag, int maxiter, int mem, double ftol, double gtol, double fd_step, double* x,
                              double* fun, int* nit, int* nfev, int* status)
{
    if (!cb || d < 1 || K < 1 || K > CARMA_KBANDS_MAX || B < 0 || !lo || !hi || mem < 1 || mem > 64 || maxiter < 0) return CARMA_EINVAL;
    auto dens = [cb, user](const double* thx, int npts, double* out) { return cb(thx, npts, out, user); };
    return carma::mband_mle_run(dens, d, K, x0, B, lo, hi, fixed_lag, maxiter, mem, ftol, gtol, fd_step, x, fun, nit, nfev, status);
}

// carma_bands_create's argument checks: 0 and an empty message, or CARMA_EINVAL and the message
extern "C" int mband_check_create_host(const double* time, const double* y, const double* yerr, const long* offsets, int K, int p, int q,
                                       const double* lag_lo, const double* lag_hi, char* msg, int len)
{
    const std::string s = carma::mband_check_create(time, y, yerr, offsets, K, p, q, lag_lo, lag_hi);
    snprintf(msg, len, "%s", s.c_str());
    return s.empty() ? CARMA_OK : CARMA_EINVAL;
}
