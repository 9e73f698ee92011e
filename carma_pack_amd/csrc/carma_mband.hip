// carma_mband.hip -- one CARMA process in K bands with a lag, a scale and an offset per band: the one-evaluation-per-lane
// log-density kernel that merges the bands on the fly (carma_mband.h), the context of the C ABI (carma_bands_*) and the
// lock-step optimiser on the extended parameter vector (mle_loop with the evaluator of carma_mband_plan.h).
//
// A launch is ceil(B / 64) workgroups of one wave, as k_logdens_carma_lane_ms; nothing but the series' length is wave-uniform,
// so the records come in with per-lane vector loads and every lane computes its own transition factors.  The work arrays of
// the merge ([K][64] per array, carma_mband.h) are dynamic LDS: 2816 bytes per band, 24 KiB with the tables at K = 8.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "grp_device.h"
#include "carma_core.h"
#include "carma_lane.h"
#include "carma_mband.h"
#include "carma_host.h"
#include "carma_mband_plan.h"
#include "carma_mband_ctx.h"

namespace carma {

static_assert(MBAND_KMAX == CARMA_KBANDS_MAX, "carma_mband.h and include/carma_mi355.h disagree on the number of bands");

template <int P>
__global__ __launch_bounds__(64) void k_logdens_carma_mband(const double* __restrict__ theta, int dx, int q, int K, int N,
                                                           const double4* __restrict__ rec, const int* __restrict__ boff,
                                                           const double* __restrict__ lagbox, Prior pr, int B, int ignore_prior,
                                                           double* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];   // all LDS is dynamic (mband_lds_bytes)
    const int lane = threadIdx.x;
    MbandWork wk;
    const double* s_tab = mband_lds_carve(s_dyn, K, K, lane, boff, 0, wk);
    long e = (long)blockIdx.x * 64 + lane;
    const bool live = e < B;
    if (!live) e = (long)blockIdx.x * 64;                    // pad lanes recompute the wave's first evaluation and write nothing
    const double ll = logdensity_mband_lane<P>(theta + e * dx, q, K, N, rec, lagbox, pr, ignore_prior, s_tab, wk);
    if (live) out[e] = ll;
}

static hipError_t launch_logdens_mband(int p, const double* theta, int B, int dx, int q, int K, int N, const double4* rec,
                                       const int* boff, const double* lagbox, const Prior& pr, int ignore_prior, double* out,
                                       hipStream_t st)
{
    if (B <= 0) return hipSuccess;
    const dim3 grid((unsigned)((B + 63) / 64)), block(64);
    const size_t lds = mband_lds_bytes(K);
    auto go = [&](auto P) {
        hipLaunchKernelGGL((k_logdens_carma_mband<decltype(P)::value>), grid, block, lds, st, theta, dx, q, K, N, rec, boff, lagbox, pr, B,
                           ignore_prior, out);
        return hipGetLastError();
    };
    if (p == 1) return go(std::integral_constant<int, 1>{});   // (for_order starts at 2: CAR(1) is the generic body at P = 1 here)
    return for_order(p, hipErrorInvalidValue, go);
}

}  // namespace carma

using namespace carma;

extern "C" {

carma_bands* carma_bands_create(const double* time, const double* y, const double* yerr, const long* offsets, int nbands, int p,
                                int q, const double* lag_lo, const double* lag_hi, double max_stdev, int device)
{
    const std::string bad = mband_check_create(time, y, yerr, offsets, nbands, p, q, lag_lo, lag_hi);
    if (!bad.empty()) {
        set_error("carma_bands_create: %s", bad.c_str());
        return nullptr;
    }
    // (host only: all argument errors come before any device work)
    const int K = nbands;
    Bctx* c = new Bctx();
    c->device = device;
    c->p = p;
    c->q = q;
    c->d = 3 + p + q;
    c->K = K;
    c->dx = mband_dim(c->d, K);
    if (!mband_prepare(time, y, yerr, offsets, K, lag_lo, lag_hi, &max_stdev, c->o)) {
        set_error("carma_bands_create: fewer than 2 data after the duplicate times of each band are dropped");
        delete c;
        return nullptr;
    }
    if (select_device(device) != CARMA_OK) {
        delete c;
        return nullptr;
    }
    hipError_t e = to_device(c->d_rec, c->o.rec);
    if (e == hipSuccess) e = to_device(c->d_boff, c->o.boff);
    if (e == hipSuccess) e = to_device(c->d_lagbox, c->o.lagbox, sizeof(double) * 2 * MBAND_KMAX);
    std::vector<double>().swap(c->o.rec);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        hip_fail(e, "carma_bands_create");
        carma_bands_destroy(reinterpret_cast<carma_bands*>(c));
        return nullptr;
    }
    return reinterpret_cast<carma_bands*>(c);
}

void carma_bands_destroy(carma_bands* h)
{
    if (!h) return;
    Bctx* c = reinterpret_cast<Bctx*>(h);
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;                                                 // (the DevMem members release their buffers)
}

int carma_bands_dim(const carma_bands* h) { return h ? reinterpret_cast<const Bctx*>(h)->dx : CARMA_EINVAL; }
int carma_bands_nbands(const carma_bands* h) { return h ? reinterpret_cast<const Bctx*>(h)->K : CARMA_EINVAL; }

int carma_bands_n(const carma_bands* h, int b)
{
    if (!h || b < 0 || b >= reinterpret_cast<const Bctx*>(h)->K) return CARMA_EINVAL;
    return reinterpret_cast<const Bctx*>(h)->o.n[b];
}

int carma_bands_get_prior(const carma_bands* h, double* out3)
{
    if (!h || !out3) return CARMA_EINVAL;
    prior_out3(reinterpret_cast<const Bctx*>(h)->o.pr, out3);
    return CARMA_OK;
}

int carma_bands_logdensity_batch_dev(carma_bands* h, const double* d_theta, int B, int ignore_prior, double* d_out, void* stream)
{
    if (!h || !d_theta || !d_out || B < 0) {
        set_error("carma_bands_logdensity_batch_dev: bad argument");
        return CARMA_EINVAL;
    }
    if (B == 0) return CARMA_OK;
    Bctx* c = reinterpret_cast<Bctx*>(h);
    (void)hipGetLastError();   // HIP's last-error is sticky: drop anything left by earlier calls
    const hipError_t e = launch_logdens_mband(c->p, d_theta, B, c->dx, c->q, c->K, c->o.N, c->d_rec.as<const double4>(),
                                              c->d_boff.as<const int>(), c->d_lagbox.as<const double>(), c->o.pr, ignore_prior, d_out,
                                              reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "carma_bands_logdensity_batch_dev: launch");
    return CARMA_OK;
}

int carma_bands_logdensity_batch(carma_bands* h, const double* theta, int B, int ignore_prior, double* out)
{
    if (!h || B < 0 || (B > 0 && (!theta || !out))) {
        set_error("carma_bands_logdensity_batch: bad argument");
        return CARMA_EINVAL;
    }
    if (B == 0) return CARMA_OK;
    Bctx* c = reinterpret_cast<Bctx*>(h);
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    e = c->d_theta.need(sizeof(double) * (size_t)B * c->dx);
    if (e == hipSuccess) e = c->d_out.need(sizeof(double) * (size_t)B);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->d_theta.as<void>(), theta, sizeof(double) * (size_t)B * c->dx, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return hip_fail(e, "carma_bands_logdensity_batch: H2D");
    int rc = carma_bands_logdensity_batch_dev(h, c->d_theta.as<double>(), B, ignore_prior, c->d_out.as<double>(), c->stream);
    if (rc == CARMA_OK) {
        e = hipMemcpyAsync(out, c->d_out.as<void>(), sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) rc = hip_fail(e, "carma_bands_logdensity_batch: D2H");
    }
    // (also after a failure: the enqueued copies read and write the caller's arrays)
    e = hipStreamSynchronize(c->stream);
    if (rc == CARMA_OK && e != hipSuccess) rc = hip_fail(e, "carma_bands_logdensity_batch");
    return rc;
}

int carma_bands_mle_batched(carma_bands* h, const double* x0, int B, const double* lo_in, const double* hi_in, const double* fixed_lag,
                            int maxiter, int mem, double ftol, double gtol, double fd_step, int ignore_prior, double* x_out,
                            double* fun_out, int* nit_out, int* nfev_out, int* status_out)
{
    if (!h || B < 0 || (B > 0 && (!x0 || !x_out || !fun_out)) || mem < 1 || mem > 64 || maxiter < 0) {
        set_error("carma_bands_mle_batched: bad argument");
        return CARMA_EINVAL;
    }
    Bctx* c = reinterpret_cast<Bctx*>(h);
    const int K = c->K, d = c->d, dx = c->dx;
    const long nf = mband_fixed_lag_bad(fixed_lag, B, K);
    if (nf >= 0) {
        set_error("carma_bands_mle_batched: fixed_lag of start %ld, band %ld is not finite", nf / (K - 1), nf % (K - 1) + 1);
        return CARMA_EINVAL;
    }
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> lo, hi;
    fill_box(lo_in, dx, -inf, lo);
    fill_box(hi_in, dx, inf, hi);
    int band = 0;
    if (mband_cut_boxes(lo.data(), hi.data(), nullptr, 1, d, K, c->o.lagbox.data(), fixed_lag != nullptr, &band) >= 0) {
        set_error("carma_bands_mle_batched: lo / hi leave nothing of the lag box of band %d", band);
        return CARMA_EINVAL;
    }
    auto dens = [h, ignore_prior](const double* thx, int npts, double* out) {
        return carma_bands_logdensity_batch(h, thx, npts, ignore_prior, out);
    };
    return mband_mle_run(dens, d, K, x0, B, lo.data(), hi.data(), fixed_lag, maxiter, mem, ftol, gtol, fd_step, x_out, fun_out,
                         nit_out, nfev_out, status_out);
}

}  // extern "C"
