// carma_mseries.hip -- MANY series in one launch: the one-evaluation-per-lane log-density kernels with the series chosen per
// wave from a table, and the multi-series context of the C ABI (carma_mctx_*).  The launch plan that builds the table is
// host-only code in carma_mseries_plan.h; the item calls of a set are in carma_mitems.hip, its sampler in carma_mpt.hip.
//
// A survey fits thousands of light curves, each on its own; a launch per series leaves most of the chip idle (one series
// rarely supplies the ~25 000 evaluations the lane kernel needs to fill 256 CUs).  Here all series of a set live in ONE
// buffer in HBM and a launch carries evaluations of any of them:
//   - one wave per workgroup, as k_logdens_carma_lane; wave w works on series wave_series[w] -- an index that derives from
//     blockIdx.x alone, so the series' offset, length and prior bounds are wave-uniform and come in with scalar loads, and so
//     do the series records in the filter loop, exactly as in the single-series kernel;
//   - lane l of wave w evaluates parameter vector eval_idx[64 w + l] and writes out[eval_idx[64 w + l]] (the caller's order);
//     pad lanes (eval_idx = -1) compute a copy of the wave's first evaluation and write nothing;
//   - the filter is logdensity_lane / logdensity_car1 unchanged, and REPDT is decided per series as carma_ctx_create decides
//     it: a series gives the same bits as the single-series lane kernel on it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "grp_device.h"
#include "carma_core.h"
#include "carma_lane.h"
#include "carma_mseries.h"

namespace carma {

template <int P, bool REPDT>
__global__ __launch_bounds__(64) void k_logdens_carma_lane_ms(const double* __restrict__ theta, int d, int q,
                                                             const double4* __restrict__ records, const long* __restrict__ off,
                                                             const int* __restrict__ nser, const Prior* __restrict__ prs,
                                                             const int* __restrict__ wave_series, const int* __restrict__ eval_idx,
                                                             int ignore_prior, double* __restrict__ out)
{
    __shared__ double s_tab[MATH_TAB_N];                     // tables of the table-based exp / sincos (carma_math.h)
    math_tab_fill(s_tab);
    __syncthreads();
    const int s = wave_series[blockIdx.x];                   // wave-uniform: scalar loads of the series' record
    const double4* series = records + off[s];
    const int n = nser[s];
    const Prior pr = prs[s];
    const int* ew = eval_idx + (long)blockIdx.x * 64;
    int e = ew[threadIdx.x];
    const bool live = e >= 0;
    if (!live) e = ew[0];                                    // (lane 0 of a wave is always live)
    const double ll = logdensity_lane<P, REPDT>(theta + (long)e * d, q, series, n, pr, ignore_prior, s_tab);
    if (live) out[e] = ll;
}

__global__ __launch_bounds__(64) void k_logdens_car1_ms(const double* __restrict__ theta, const double4* __restrict__ records,
                                                        const long* __restrict__ off, const int* __restrict__ nser,
                                                        const Prior* __restrict__ prs, const int* __restrict__ wave_series,
                                                        const int* __restrict__ eval_idx, double* __restrict__ out)
{
    const int s = wave_series[blockIdx.x];
    const double4* series = records + off[s];
    const int n = nser[s];
    const Prior pr = prs[s];
    const int* ew = eval_idx + (long)blockIdx.x * 64;
    int e = ew[threadIdx.x];
    const bool live = e >= 0;
    if (!live) e = ew[0];
    const double ll = logdensity_car1(theta + 4L * e, series, n, pr);
    if (live) out[e] = ll;
}

// nwaves waves of the table (wave_series[nwaves], eval_idx[64 nwaves]) in one launch
static hipError_t launch_logdens_ms(int p, bool repdt, const double* theta, int d, int q, const double4* records, const long* off,
                                    const int* nser, const Prior* prs, const int* wave_series, const int* eval_idx, long nwaves,
                                    int ignore_prior, double* out, hipStream_t st)
{
    if (nwaves <= 0) return hipSuccess;
    const dim3 grid((unsigned)nwaves), block(64);
    if (p == 1) {
        hipLaunchKernelGGL(k_logdens_car1_ms, grid, block, 0, st, theta, records, off, nser, prs, wave_series, eval_idx, out);
        return hipGetLastError();
    }
    return for_order(p, hipErrorInvalidValue, [&](auto P) {
        if (repdt)
            hipLaunchKernelGGL((k_logdens_carma_lane_ms<decltype(P)::value, true>), grid, block, 0, st, theta, d, q, records, off, nser,
                               prs, wave_series, eval_idx, ignore_prior, out);
        else
            hipLaunchKernelGGL((k_logdens_carma_lane_ms<decltype(P)::value, false>), grid, block, 0, st, theta, d, q, records, off, nser,
                               prs, wave_series, eval_idx, ignore_prior, out);
        return hipGetLastError();
    });
}

}  // namespace carma

using namespace carma;

extern "C" {

carma_mctx* carma_mctx_create(const double* time, const double* y, const double* yerr, const long* offsets, int nseries, int p,
                              int q, const double* max_stdev, int device)
{
    if (!time || !y || !yerr || !offsets || nseries < 1) {
        set_error("carma_mctx_create: need nseries >= 1 and non-null arrays (got nseries=%d)", nseries);
        return nullptr;
    }
    if (p < 1 || p > CARMA_PMAX || q < 0 || (p == 1 && q != 0) || (p > 1 && q >= p)) {
        set_error("carma_mctx_create: need 1 <= p <= %d and q < p (got p=%d q=%d)", CARMA_PMAX, p, q);
        return nullptr;
    }
    if (offsets[0] != 0) {
        set_error("carma_mctx_create: offsets[0] must be 0 (got %ld)", offsets[0]);
        return nullptr;
    }
    for (int s = 0; s < nseries; s++) {
        if (offsets[s + 1] < offsets[s]) {
            set_error("carma_mctx_create: offsets must be non-decreasing (offsets[%d]=%ld > offsets[%d]=%ld)", s, offsets[s], s + 1,
                      offsets[s + 1]);
            return nullptr;
        }
        if (offsets[s + 1] - offsets[s] > 0x7fffffffL - P3L_PAD_RECORDS) {
            set_error("carma_mctx_create: series %d is longer than an int can count", s);
            return nullptr;
        }
    }
    // every series prepared as carma_ctx_create prepares one (host only: all argument errors come before any device work)
    Mctx* c = new Mctx();
    c->device = device;
    c->p = p;
    c->q = q;
    c->d = (p == 1) ? 4 : 3 + p + q;
    c->S = nseries;
    c->hoff.assign(nseries + 1, 0);
    c->off.resize(nseries);
    c->n.resize(nseries);
    c->pr.resize(nseries);
    c->repdt.resize(nseries);
    std::vector<std::vector<double>> packed(nseries);
    long rec_total = 0;
    for (int s = 0; s < nseries; s++) {
        const long a = offsets[s], b = offsets[s + 1];
        std::vector<double> ts(time + a, time + b), ys(y + a, y + b), es(yerr + a, yerr + b);
        sort_dedup(ts, ys, es);
        const long ns = (long)ts.size();
        if (ns < 2) {
            set_error("carma_mctx_create: series %d has fewer than 2 distinct times", s);
            delete c;
            return nullptr;
        }
        const double ms = max_stdev ? max_stdev[s] : default_max_stdev(y + a, b - a);   // (of the series as given)
        c->pr[s].measerr_dof = 50.0;   // src/include/carpack.hpp:63
        set_prior_bounds(c->pr[s], ts.data(), ns, ms);
        packed[s] = pack_series(ts, ys, es);
        c->repdt[s] = series_repeated_dt(packed[s].data(), ns);
        c->n[s] = (int)ns;
        c->off[s] = rec_total;
        rec_total += (ns + P3L_PAD_RECORDS + 1) / 2 * 2;     // records and pad records, the next series on a 64-byte boundary
        c->hoff[s + 1] = c->hoff[s] + ns;
        c->t.insert(c->t.end(), ts.begin(), ts.end());
        c->y.insert(c->y.end(), ys.begin(), ys.end());
        c->yerr.insert(c->yerr.end(), es.begin(), es.end());
    }
    if (select_device(device) != CARMA_OK) {
        delete c;
        return nullptr;
    }
    std::vector<double> rec((size_t)rec_total * 4, 0.0);
    for (int s = 0; s < nseries; s++) {
        const size_t nr = (size_t)c->n[s] + P3L_PAD_RECORDS;         // the records and pads of pack_series (its tail arrays stay out)
        std::memcpy(&rec[(size_t)c->off[s] * 4], packed[s].data(), sizeof(double) * 4 * nr);
        std::vector<double>().swap(packed[s]);
    }
    hipError_t e = to_device(c->d_rec, rec);
    if (e == hipSuccess) e = to_device(c->d_off, c->off);
    if (e == hipSuccess) e = to_device(c->d_n, c->n);
    if (e == hipSuccess) e = to_device(c->d_pr, c->pr);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        hip_fail(e, "carma_mctx_create");
        carma_mctx_destroy(reinterpret_cast<carma_mctx*>(c));
        return nullptr;
    }
    return reinterpret_cast<carma_mctx*>(c);
}

void carma_mctx_destroy(carma_mctx* h)
{
    if (!h) return;
    Mctx* c = reinterpret_cast<Mctx*>(h);
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;                                                 // (its members release their buffers, the sampler state among them)
}

int carma_mctx_nseries(const carma_mctx* h) { return h ? reinterpret_cast<const Mctx*>(h)->S : CARMA_EINVAL; }
int carma_mctx_dim(const carma_mctx* h) { return h ? reinterpret_cast<const Mctx*>(h)->d : CARMA_EINVAL; }

int carma_mctx_n(const carma_mctx* h, int s)
{
    if (!h || s < 0 || s >= reinterpret_cast<const Mctx*>(h)->S) return CARMA_EINVAL;
    return reinterpret_cast<const Mctx*>(h)->n[s];
}

int carma_mctx_get_data(const carma_mctx* h, int s, double* time, double* y, double* yerr)
{
    if (!h || s < 0 || s >= reinterpret_cast<const Mctx*>(h)->S) return CARMA_EINVAL;
    const Mctx* c = reinterpret_cast<const Mctx*>(h);
    const size_t a = (size_t)c->hoff[s], n = (size_t)c->n[s];
    if (time) std::memcpy(time, c->t.data() + a, sizeof(double) * n);
    if (y) std::memcpy(y, c->y.data() + a, sizeof(double) * n);
    if (yerr) std::memcpy(yerr, c->yerr.data() + a, sizeof(double) * n);
    return CARMA_OK;
}

int carma_mctx_get_prior(const carma_mctx* h, int s, double* out3)
{
    if (!h || !out3 || s < 0 || s >= reinterpret_cast<const Mctx*>(h)->S) return CARMA_EINVAL;
    prior_out3(reinterpret_cast<const Mctx*>(h)->pr[s], out3);
    return CARMA_OK;
}

int carma_mlogdensity_batch(carma_mctx* h, const double* theta, const int* series, int B, int ignore_prior, double* out)
{
    if (!h || B < 0 || (B > 0 && (!theta || !series || !out))) {
        set_error("carma_mlogdensity_batch: bad argument");
        return CARMA_EINVAL;
    }
    if (B == 0) return CARMA_OK;
    Mctx* c = reinterpret_cast<Mctx*>(h);
    const int d = c->d;
    // the plan's first w_plain waves are the REPDT = false launch, the others the REPDT = true one
    auto enqueue = [&](const double* d_theta, const int* d_wser, const int* d_eidx, long W, long w_plain, double* d_out, hipStream_t st) {
        hipError_t e = launch_logdens_ms(c->p, false, d_theta, d, c->q, c->rec(), c->offs(), c->ns(), c->prs(), d_wser, d_eidx, w_plain,
                                         ignore_prior, d_out, st);
        if (e == hipSuccess)
            e = launch_logdens_ms(c->p, true, d_theta, d, c->q, c->rec(), c->offs(), c->ns(), c->prs(), d_wser + w_plain,
                                  d_eidx + (size_t)w_plain * 64, W - w_plain, ignore_prior, d_out, st);
        return e;
    };
    return wave_batch_run(c->wb, "carma_mlogdensity_batch", c->device, c->stream, theta, d, series, B, c->S, "series", "nseries",
                          c->n.data(), c->repdt.data(), out, enqueue);
}

int carma_mlogdensity_kernel_name(const carma_mctx* h, char* buf, int len)
{
    if (!h || !buf || len < 1) return CARMA_EINVAL;
    const Mctx* c = reinterpret_cast<const Mctx*>(h);
    const int r = c->p == 1 ? snprintf(buf, len, "k_logdens_car1_ms") : snprintf(buf, len, "k_logdens_carma_lane_ms<%d>", c->p);
    return r > 0 ? CARMA_OK : CARMA_EINVAL;
}

}  // extern "C"
