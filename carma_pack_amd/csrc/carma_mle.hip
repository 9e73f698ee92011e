// carma_mle.hip -- lock-step bounded quasi-Newton minimiser of -LogDensity for MANY starts at once.
//
// carma_pack's get_mle runs `ntrials` separate scipy L-BFGS-B searches and crosses the FFI once per function evaluation
// (reference carma_pack.py:92-129,195-260).  On the GPU one log-density costs the same as a thousand, so all starts are
// advanced together: per iteration ONE batched launch evaluates the central-difference stencils of every active start
// (B x (2d+1) points) and one more evaluates eight consecutive backtracking step lengths of every start.  This file is
// the host side of that loop in C++ (the Python prototype, carma_pack_amd/batched_opt.py, spent as long in the
// interpreter as in the launches: 5.4 of 13.9 s of choose_order(pmax=7, ntrials=100)); same algorithm, same constants.
//
// The update is a projected L-BFGS step (two-loop recursion per start; variables sitting on a bound with the gradient
// pointing outwards are frozen) with an Armijo backtracking line search; stopping rules mirror L-BFGS-B's defaults
// (projected gradient <= gtol, or `patience` consecutive iterations with a relative decrease <= ftol after one restart of
// the quasi-Newton memory).
//
// The loop itself (mle_loop, fill_box, the constants) lives in carma_mle_loop.h, host C++ without a HIP include and templated on
// its evaluator: this file holds the two evaluators that launch the log-density kernels and the C entry points; the tests
// instantiate the same loop on objectives with known answers (tests/mleloop/).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/carma_mi355.h"
#include "carma_host.h"
#include "carma_mle_loop.h"

using namespace carma;

namespace {

// An evaluator: operator()(pts, owner, npts) sets out[k] = f(pts[k]) = -LogDensity (non-finite -> BIG); owner[k] is the start
// point k belongs to, filled by the loop only where PER_START is true.
struct Eval {                    // one series (carma_ctx)
    static constexpr bool PER_START = false;
    carma_ctx* h;
    int ignore_prior;
    std::vector<double> out;
    int operator()(const std::vector<double>& pts, const std::vector<int>&, int npts)
    {
        out.resize((size_t)npts);
        if (npts == 0) return CARMA_OK;
        const int rc = carma_logdensity_batch(h, pts.data(), npts, ignore_prior, out.data());
        if (rc != CARMA_OK) return rc;
        for (int i = 0; i < npts; i++) {
            const double f = -out[i];
            out[i] = std::isfinite(f) ? f : BIG;
        }
        return CARMA_OK;
    }
};

struct EvalMs {                  // many series (carma_mctx): every point on its start's series
    static constexpr bool PER_START = true;
    carma_mctx* h;
    const int* series;           // [B] series of each start
    int ignore_prior;
    std::vector<double> out;
    std::vector<int> ser;
    int operator()(const std::vector<double>& pts, const std::vector<int>& owner, int npts)
    {
        out.resize((size_t)npts);
        if (npts == 0) return CARMA_OK;
        ser.resize((size_t)npts);
        for (int i = 0; i < npts; i++) ser[i] = series[owner[i]];
        const int rc = carma_mlogdensity_batch(h, pts.data(), ser.data(), npts, ignore_prior, out.data());
        if (rc != CARMA_OK) return rc;
        for (int i = 0; i < npts; i++) {
            const double f = -out[i];
            out[i] = std::isfinite(f) ? f : BIG;
        }
        return CARMA_OK;
    }
};

}  // namespace

extern "C" int carma_mle_batched(carma_ctx* h, const double* x0, int B, const double* lo_in, const double* hi_in, int maxiter,
                                 int mem, double ftol, double gtol, double fd_step, int ignore_prior, double* x_out,
                                 double* fun_out, int* nit_out, int* nfev_out, int* status_out)
{
    if (!h || !x0 || B < 0 || !x_out || !fun_out || mem < 1 || mem > 64 || maxiter < 0) {
        set_error("carma_mle_batched: bad argument");
        return CARMA_EINVAL;
    }
    const int d = carma_ctx_dim(h);
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> lo, hi;
    fill_box(lo_in, d, -inf, lo);
    fill_box(hi_in, d, inf, hi);
    Eval fun{h, ignore_prior, {}};
    return mle_loop(fun, d, x0, B, lo.data(), hi.data(), 0, maxiter, mem, ftol, gtol, fd_step, x_out, fun_out, nit_out, nfev_out,
                    status_out);
}

extern "C" int carma_mle_batched_ms(carma_mctx* h, const double* x0, const int* series, int B, const double* lo_in,
                                    const double* hi_in, int maxiter, int mem, double ftol, double gtol, double fd_step,
                                    int ignore_prior, double* x_out, double* fun_out, int* nit_out, int* nfev_out, int* status_out)
{
    if (!h || B < 0 || (B > 0 && (!x0 || !series || !x_out || !fun_out)) || mem < 1 || mem > 64 || maxiter < 0) {
        set_error("carma_mle_batched_ms: bad argument");
        return CARMA_EINVAL;
    }
    const int S = carma_mctx_nseries(h);
    for (int i = 0; i < B; i++)
        if (series[i] < 0 || series[i] >= S) {
            set_error("carma_mle_batched_ms: series[%d] = %d out of range (nseries = %d)", i, series[i], S);
            return CARMA_EINVAL;
        }
    const int d = carma_mctx_dim(h);
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> lo, hi;
    fill_box(lo_in, (size_t)B * d, -inf, lo);
    fill_box(hi_in, (size_t)B * d, inf, hi);
    EvalMs fun{h, series, ignore_prior, {}, {}};
    return mle_loop(fun, d, x0, B, lo.data(), hi.data(), (size_t)d, maxiter, mem, ftol, gtol, fd_step, x_out, fun_out, nit_out,
                    nfev_out, status_out);
}
