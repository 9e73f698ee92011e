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

// dynamic LDS of a workgroup: tables, work arrays, band offsets (padded to 16 ints)
static size_t mband_lds_bytes(int K) { return sizeof(double) * MATH_TAB_N + MbandWork::bytes(K) + sizeof(int) * 16; }

template <int P>
__global__ __launch_bounds__(64) void k_logdens_carma_mband(const double* __restrict__ theta, int dx, int q, int K, int N,
                                                           const double4* __restrict__ rec, const int* __restrict__ boff,
                                                           const double* __restrict__ lagbox, Prior pr, int B, int ignore_prior,
                                                           double* __restrict__ out)
{
    // all LDS is dynamic, every carve a multiple of 16 bytes: the tables of the table-based exp / sincos (carma_math.h), the work
    // arrays [5][K][64] doubles and [K][64] ints, the band offsets
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    const int lane = threadIdx.x;
    const size_t KL = (size_t)K * MBAND_LANES;
    double* s_tab = s_dyn;
    double* s_work = s_dyn + MATH_TAB_N;
    int* s_pos = reinterpret_cast<int*>(s_work + 5 * KL);
    int* s_boff = s_pos + KL;
    math_tab_fill(s_tab);
    if (lane <= K) s_boff[lane] = boff[lane];
    __syncthreads();
    MbandWork wk;
    wk.y = s_work + lane;
    wk.e2 = s_work + KL + lane;
    wk.a = s_work + 2 * KL + lane;
    wk.mu = s_work + 3 * KL + lane;
    wk.lag = s_work + 4 * KL + lane;
    wk.pos = s_pos + lane;
    wk.boff = s_boff;
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
    // every band prepared as carma_ctx_create prepares a series (host only: all argument errors come before any device work)
    const int K = nbands;
    std::vector<std::vector<double>> ts(K), ys(K), es(K);
    Bctx* c = new Bctx();
    c->device = device;
    c->p = p;
    c->q = q;
    c->d = 3 + p + q;
    c->K = K;
    c->dx = mband_dim(c->d, K);
    c->n.resize(K);
    for (int b = 0; b < K; b++) {
        ts[b].assign(time + offsets[b], time + offsets[b + 1]);
        ys[b].assign(y + offsets[b], y + offsets[b + 1]);
        es[b].assign(yerr + offsets[b], yerr + offsets[b + 1]);
        sort_dedup(ts[b], ys[b], es[b]);
        c->n[b] = (int)ts[b].size();
        c->N += c->n[b];
    }
    if (c->N < 2) {
        set_error("carma_bands_create: fewer than 2 data after the duplicate times of each band are dropped");
        delete c;
        return nullptr;
    }
    c->pr.measerr_dof = 50.0;   // src/include/carpack.hpp:63
    set_prior_bounds(c->pr, ts[0].data(), c->n[0], max_stdev);
    for (int b = 0; b + 1 < K; b++) {
        c->lagbox.push_back(lag_lo[b]);
        c->lagbox.push_back(lag_hi[b]);
    }
    std::vector<double> rec;
    mband_pack(ts, ys, es, rec, c->boff);
    c->t0 = ts[0][0];                                         // (as mband_pack takes it: requested times get the same shift)
    for (int b = 1; b < K; b++) c->t0 = std::min(c->t0, ts[b][0]);
    c->ts = ts;
    c->ys = ys;
    if (select_device(device) != CARMA_OK) {
        delete c;
        return nullptr;
    }
    hipError_t e = c->d_rec.alloc(sizeof(double) * rec.size());
    if (e == hipSuccess) e = hipMemcpy(c->d_rec.as<void>(), rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = c->d_boff.alloc(sizeof(int) * (K + 1));
    if (e == hipSuccess) e = hipMemcpy(c->d_boff.as<void>(), c->boff.data(), sizeof(int) * (K + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = c->d_lagbox.alloc(sizeof(double) * 2 * MBAND_KMAX);
    if (e == hipSuccess && K > 1)
        e = hipMemcpy(c->d_lagbox.as<void>(), c->lagbox.data(), sizeof(double) * c->lagbox.size(), hipMemcpyHostToDevice);
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
    return reinterpret_cast<const Bctx*>(h)->n[b];
}

int carma_bands_get_prior(const carma_bands* h, double* out3)
{
    if (!h || !out3) return CARMA_EINVAL;
    const Prior& pr = reinterpret_cast<const Bctx*>(h)->pr;
    out3[0] = pr.max_stdev;
    out3[1] = pr.max_freq;
    out3[2] = pr.min_freq;
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
    const hipError_t e = launch_logdens_mband(c->p, d_theta, B, c->dx, c->q, c->K, c->N, c->d_rec.as<const double4>(),
                                              c->d_boff.as<const int>(), c->d_lagbox.as<const double>(), c->pr, ignore_prior, d_out,
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
    if (fixed_lag)
        for (long i = 0; i < (long)B * (K - 1); i++)
            if (!std::isfinite(fixed_lag[i])) {
                set_error("carma_bands_mle_batched: fixed_lag of start %ld, band %ld is not finite", i / (K - 1), i % (K - 1) + 1);
                return CARMA_EINVAL;
            }
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> lo, hi;
    fill_box(lo_in, dx, -inf, lo);
    fill_box(hi_in, dx, inf, hi);
    for (int b = 1; b < K; b++) {                             // a lag never leaves its box, with or without the prior
        lo[d + 3 * (b - 1)] = std::max(lo[d + 3 * (b - 1)], c->lagbox[2 * (b - 1)]);
        hi[d + 3 * (b - 1)] = std::min(hi[d + 3 * (b - 1)], c->lagbox[2 * (b - 1) + 1]);
        if (!fixed_lag && lo[d + 3 * (b - 1)] > hi[d + 3 * (b - 1)]) {
            set_error("carma_bands_mle_batched: lo / hi leave nothing of the lag box of band %d", b);
            return CARMA_EINVAL;
        }
    }
    auto dens = [h, ignore_prior](const double* thx, int npts, double* out) {
        return carma_bands_logdensity_batch(h, thx, npts, ignore_prior, out);
    };
    return mband_mle_run(dens, d, K, x0, B, lo.data(), hi.data(), fixed_lag, maxiter, mem, ftol, gtol, fd_step, x_out, fun_out,
                         nit_out, nfev_out, status_out);
}

}  // extern "C"
