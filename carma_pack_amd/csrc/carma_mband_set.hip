// carma_mband_set.hip -- MANY multi-band objects in one launch: the one-evaluation-per-lane log-density kernel of carma_mband.hip
// with the object chosen per wave from a table, the context of the C ABI (carma_bandset_*) and the lock-step optimiser over the
// starts of all objects (mle_loop with the evaluator of carma_mband_set_plan.h).
//
// A survey field is seen in the same K filters, a lens-monitoring campaign adds an object per system; a launch per object and
// optimiser step holds a few waves on a chip of 256 CUs and pays its own copies and stream sync.  Here the S objects of a set
// -- K, p and q shared by all of them, so dx is one number; an object that lacks a band belongs to another set -- live in ONE
// record buffer, each prepared by the single object's preparer (mband_prepare), and a launch carries evaluations of any of them:
//   - one wave per workgroup, as k_logdens_carma_mband; wave w works on object wave_obj[w], an index that derives from
//     blockIdx.x alone: the record base, the band offsets in LDS, the trip count N, the lag boxes and the prior bounds stay
//     wave-uniform, as the single-object kernel has them;
//   - lane l of wave w evaluates parameter vector eval_idx[64 w + l] and writes out[eval_idx[64 w + l]] (the caller's order);
//     pad lanes (eval_idx = -1; they only trail, lane 0 is live) recompute the wave's first evaluation and write nothing;
//   - the body is logdensity_mband_lane<P> unchanged: an evaluation has the bits carma_bands_logdensity_batch gives for it on
//     a handle of its object alone.
// The cost of that design: a wave never mixes objects, so an object with ONE evaluation in a launch occupies a wave of which 63
// lanes are pads (the optimiser's launches carry >= 2 dx + 1 evaluations a start, the sets it is meant for many starts each).
// The launch plan is that of carma_mlogdensity_batch (carma_mseries_plan.h), with the objects' N as the lengths.
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
#include "carma_mband_set_ctx.h"

namespace carma {

template <int P>
__global__ __launch_bounds__(64) void k_logdens_carma_mband_ms(const double* __restrict__ theta, int dx, int q, int K,
                                                              const double4* __restrict__ rec, const long* __restrict__ off,
                                                              const int* __restrict__ boff, const int* __restrict__ nobj,
                                                              const double* __restrict__ lagbox, const Prior* __restrict__ prs,
                                                              const int* __restrict__ wave_obj, const int* __restrict__ eval_idx,
                                                              int ignore_prior, double* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];   // all LDS is dynamic (mband_lds_bytes)
    const int lane = threadIdx.x;
    // wave-uniform: everything of the object derives from blockIdx.x alone.  These loads stand ahead of the carve and its barrier,
    // where the compiler can still show that nothing has written the tables: they stay scalar loads, the values in SGPRs
    const int s = wave_obj[blockIdx.x];
    const double4* orec = rec + off[s];
    const int N = nobj[s];
    const Prior pr = prs[s];
    const double* obox = lagbox + (long)s * 2 * (K - 1);
    MbandWork wk;
    const double* s_tab = mband_lds_carve(s_dyn, K, K, lane, boff, s, wk);
    const int* ew = eval_idx + (long)blockIdx.x * 64;
    int e = ew[lane];
    const bool live = e >= 0;
    if (!live) e = ew[0];                                    // (lane 0 of a wave is always live)
    const double ll = logdensity_mband_lane<P>(theta + (long)e * dx, q, K, N, orec, obox, pr, ignore_prior, s_tab, wk);
    if (live) out[e] = ll;
}

// nwaves waves of the table (wave_obj[nwaves], eval_idx[64 nwaves]) in one launch
static hipError_t launch_logdens_mband_ms(const BSctx* c, const double* theta, const int* wave_obj, const int* eval_idx, long nwaves,
                                          int ignore_prior, double* out, hipStream_t st)
{
    if (nwaves <= 0) return hipSuccess;
    const dim3 grid((unsigned)nwaves), block(64);
    const size_t lds = mband_lds_bytes(c->K);
    auto go = [&](auto P) {
        hipLaunchKernelGGL((k_logdens_carma_mband_ms<decltype(P)::value>), grid, block, lds, st, theta, c->dx, c->q, c->K,
                           c->d_rec.as<const double4>(), c->d_off.as<const long>(), c->d_boff.as<const int>(),
                           c->d_N.as<const int>(), c->d_lagbox.as<const double>(), c->d_pr.as<const Prior>(), wave_obj, eval_idx,
                           ignore_prior, out);
        return hipGetLastError();
    };
    if (c->p == 1) return go(std::integral_constant<int, 1>{});   // (CAR(1) is the generic body at P = 1, as launch_logdens_mband)
    return for_order(c->p, hipErrorInvalidValue, go);
}

}  // namespace carma

using namespace carma;

extern "C" {

carma_bandset* carma_bandset_create(const double* time, const double* y, const double* yerr, const long* offsets, int nobjects,
                                    int nbands, int p, int q, const double* lag_lo, const double* lag_hi, const double* max_stdev,
                                    int device)
{
    const std::string bad = mbandset_check_create(time, y, yerr, offsets, nobjects, nbands, p, q, lag_lo, lag_hi);
    if (!bad.empty()) {
        set_error("carma_bandset_create: %s", bad.c_str());
        return nullptr;
    }
    // every object prepared as carma_bands_create prepares its one (host only: all argument errors come before any device work)
    const int S = nobjects, K = nbands;
    BSctx* c = new BSctx();
    c->device = device;
    c->p = p;
    c->q = q;
    c->d = 3 + p + q;
    c->K = K;
    c->S = S;
    c->dx = mband_dim(c->d, K);
    c->plain.assign(S, 0);
    const int few = mbandset_prepare(time, y, yerr, offsets, S, K, lag_lo, lag_hi, max_stdev, c->m);
    if (few >= 0) {
        set_error("carma_bandset_create: object %d: fewer than 2 data after the duplicate times of each band are dropped", few);
        delete c;
        return nullptr;
    }
    if (select_device(device) != CARMA_OK) {
        delete c;
        return nullptr;
    }
    hipError_t e = to_device(c->d_rec, c->m.rec);
    if (e == hipSuccess) e = to_device(c->d_off, c->m.off);
    if (e == hipSuccess) e = to_device(c->d_boff, c->m.boff);
    if (e == hipSuccess) e = to_device(c->d_N, c->m.N);
    if (e == hipSuccess) e = to_device(c->d_lagbox, c->m.lagbox, sizeof(double) * 2);   // (K = 1: no boxes, never read)
    if (e == hipSuccess) e = to_device(c->d_pr, c->m.pr);
    std::vector<double>().swap(c->m.rec);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        hip_fail(e, "carma_bandset_create");
        carma_bandset_destroy(reinterpret_cast<carma_bandset*>(c));
        return nullptr;
    }
    return reinterpret_cast<carma_bandset*>(c);
}

void carma_bandset_destroy(carma_bandset* h)
{
    if (!h) return;
    BSctx* c = reinterpret_cast<BSctx*>(h);
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;                                                 // (the DevMem members release their buffers)
}

int carma_bandset_nobjects(const carma_bandset* h) { return h ? reinterpret_cast<const BSctx*>(h)->S : CARMA_EINVAL; }
int carma_bandset_nbands(const carma_bandset* h) { return h ? reinterpret_cast<const BSctx*>(h)->K : CARMA_EINVAL; }
int carma_bandset_dim(const carma_bandset* h) { return h ? reinterpret_cast<const BSctx*>(h)->dx : CARMA_EINVAL; }

int carma_bandset_n(const carma_bandset* h, int s, int b)
{
    if (!h) return CARMA_EINVAL;
    const BSctx* c = reinterpret_cast<const BSctx*>(h);
    if (s < 0 || s >= c->S || b < 0 || b >= c->K) return CARMA_EINVAL;
    return c->m.n[(size_t)s * c->K + b];
}

int carma_bandset_get_prior(const carma_bandset* h, int s, double* out3)
{
    if (!h || !out3 || s < 0 || s >= reinterpret_cast<const BSctx*>(h)->S) return CARMA_EINVAL;
    prior_out3(reinterpret_cast<const BSctx*>(h)->m.pr[s], out3);
    return CARMA_OK;
}

int carma_bandset_logdensity_batch(carma_bandset* h, const double* theta, const int* object, int B, int ignore_prior, double* out)
{
    if (!h || B < 0 || (B > 0 && (!theta || !object || !out))) {
        set_error("carma_bandset_logdensity_batch: bad argument");
        return CARMA_EINVAL;
    }
    if (B == 0) return CARMA_OK;
    BSctx* c = reinterpret_cast<BSctx*>(h);
    // the launch plan of carma_mlogdensity_batch with the objects' N as the lengths and one cadence class: one launch
    auto enqueue = [&](const double* d_theta, const int* d_wobj, const int* d_eidx, long W, long, double* d_out, hipStream_t st) {
        return launch_logdens_mband_ms(c, d_theta, d_wobj, d_eidx, W, ignore_prior, d_out, st);
    };
    return wave_batch_run(c->wb, "carma_bandset_logdensity_batch", c->device, c->stream, theta, c->dx, object, B, c->S, "object",
                          "nobjects", c->m.N.data(), c->plain.data(), out, enqueue);
}

int carma_bandset_kernel_name(const carma_bandset* h, char* buf, int len)
{
    if (!h || !buf || len < 1) return CARMA_EINVAL;
    const int r = snprintf(buf, len, "k_logdens_carma_mband_ms<%d>", reinterpret_cast<const BSctx*>(h)->p);
    return r > 0 ? CARMA_OK : CARMA_EINVAL;
}

int carma_bandset_mle_batched(carma_bandset* h, const double* x0, const int* object, int B, const double* lo_in, const double* hi_in,
                              const double* fixed_lag, int maxiter, int mem, double ftol, double gtol, double fd_step,
                              int ignore_prior, double* x_out, double* fun_out, int* nit_out, int* nfev_out, int* status_out)
{
    if (!h || B < 0 || (B > 0 && (!x0 || !object || !x_out || !fun_out)) || mem < 1 || mem > 64 || maxiter < 0) {
        set_error("carma_bandset_mle_batched: bad argument");
        return CARMA_EINVAL;
    }
    BSctx* c = reinterpret_cast<BSctx*>(h);
    const int K = c->K, d = c->d, dx = c->dx;
    for (int i = 0; i < B; i++)
        if (object[i] < 0 || object[i] >= c->S) {
            set_error("carma_bandset_mle_batched: object[%d] = %d out of range (nobjects = %d)", i, object[i], c->S);
            return CARMA_EINVAL;
        }
    const long nf = mband_fixed_lag_bad(fixed_lag, B, K);
    if (nf >= 0) {
        set_error("carma_bandset_mle_batched: fixed_lag of start %ld, band %ld is not finite", nf / (K - 1), nf % (K - 1) + 1);
        return CARMA_EINVAL;
    }
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> lo, hi;
    fill_box(lo_in, (size_t)B * dx, -inf, lo);
    fill_box(hi_in, (size_t)B * dx, inf, hi);
    int band = 0;                                             // a lag never leaves its object's box, with or without the prior
    const long empty = mbandset_cut_boxes(lo.data(), hi.data(), object, B, d, K, c->m.lagbox.data(), fixed_lag != nullptr, &band);
    if (empty >= 0) {
        set_error("carma_bandset_mle_batched: start %ld: lo / hi leave nothing of the lag box of band %d of object %d", empty, band,
                  object[empty]);
        return CARMA_EINVAL;
    }
    auto dens = [h, ignore_prior](const double* thx, const int* obj, int npts, double* out) {
        return carma_bandset_logdensity_batch(h, thx, obj, npts, ignore_prior, out);
    };
    return mbandset_mle_run(dens, d, K, x0, object, B, lo.data(), hi.data(), fixed_lag, maxiter, mem, ftol, gtol, fd_step, x_out,
                            fun_out, nit_out, nfev_out, status_out);
}

}  // extern "C"
