// mleloop_host.cpp -- TEST HARNESS ONLY: the library's lock-step loop (carma_pack_amd/csrc/carma_mle_loop.h) instantiated with
// an evaluator that calls a C callback, so that tests/test_mle_loop_cpu.py can run it on objectives whose answers are known and
// see every launch it makes (points, owners, count).  Host code, built by g++ (tests/mleloop_ref.py).
#include <cmath>
#include <vector>

#include "carma_mle_loop.h"

typedef int (*mleloop_cb)(const double* pts, const int* owner, int npts, double* out, void* user);

namespace {

template <bool PS>
struct CbEval {
    static constexpr bool PER_START = PS;
    mleloop_cb cb;
    void* user;
    std::vector<double> out;
    int operator()(const std::vector<double>& pts, const std::vector<int>& owner, int npts)
    {
        out.resize((size_t)npts);
        if (npts == 0) return CARMA_OK;
        const int rc = cb(pts.data(), PS ? owner.data() : nullptr, npts, out.data(), user);
        if (rc != CARMA_OK) return rc;
        for (int i = 0; i < npts; i++)
            if (!std::isfinite(out[i])) out[i] = carma::BIG;
        return CARMA_OK;
    }
};

template <bool PS>
int run(mleloop_cb cb, void* user, int d, const double* x0, int B, const double* lo, const double* hi, int bstride, int maxiter,
        int mem, double ftol, double gtol, double fd_step, double* x, double* fun, int* nit, int* nfev, int* status)
{
    if (!cb || d < 1 || B < 0 || !lo || !hi || (bstride != 0 && bstride != d) || mem < 1 || mem > 64 || maxiter < 0)
        return CARMA_EINVAL;
    CbEval<PS> ev{cb, user, {}};
    return carma::mle_loop(ev, d, x0, B, lo, hi, (size_t)bstride, maxiter, mem, ftol, gtol, fd_step, x, fun, nit, nfev, status);
}

}  // namespace

// lo / hi: [d] with bstride 0, [B][d] with bstride d; no NULLs, unbounded = +-inf (what carma_mle.hip's fill_box hands the loop)
extern "C" int mleloop_shared(mleloop_cb cb, void* user, int d, const double* x0, int B, const double* lo, const double* hi,
                              int bstride, int maxiter, int mem, double ftol, double gtol, double fd_step, double* x, double* fun,
                              int* nit, int* nfev, int* status)
{
    return run<false>(cb, user, d, x0, B, lo, hi, bstride, maxiter, mem, ftol, gtol, fd_step, x, fun, nit, nfev, status);
}

extern "C" int mleloop_per_start(mleloop_cb cb, void* user, int d, const double* x0, int B, const double* lo, const double* hi,
                                 int bstride, int maxiter, int mem, double ftol, double gtol, double fd_step, double* x,
                                 double* fun, int* nit, int* nfev, int* status)
{
    return run<true>(cb, user, d, x0, B, lo, hi, bstride, maxiter, mem, ftol, gtol, fd_step, x, fun, nit, nfev, status);
}

extern "C" void mleloop_constants(double* big, int* ls_k, int* patience)
{
    *big = carma::BIG;
    *ls_k = carma::LS_K;
    *patience = carma::PATIENCE;
}
