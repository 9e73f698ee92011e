// carma_mband_set.hip -- MANY multi-band objects in one launch: the one-evaluation-per-lane log-density kernel of carma_mband.hip
// with the object chosen per wave from a table, the context of the C ABI (carma_bandset_*) and the lock-step optimiser over the
// starts of all objects (mle_loop with the evaluator of carma_mband_set_plan.h).
//
// A survey field is seen in the same K filters, a lens-monitoring campaign adds an object per system; a launch per object and
// optimiser step holds a few waves on a chip of 256 CUs and pays its own copies and stream sync.  Here the S objects of a set
// -- K, p and q shared by all of them, so dx is one number; an object that lacks a band belongs to another set -- live in ONE
// record buffer, each packed as carma_bands_create packs its one object, and a launch carries evaluations of any of them:
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
#include "carma_mband_set_plan.h"

namespace carma {

// A set of multi-band objects: the records of all objects in one buffer, object s as mband_pack lays it out, from record off[s]
struct BSctx {
    int device = 0;
    int p = 0, q = 0, d = 0, K = 0, dx = 0, S = 0;
    std::vector<int> n;               // [S][K] data per band after sort / dedup
    std::vector<int> N;               // [S] data per object: the trip count of its waves
    std::vector<int> boff;            // [S][K + 1] first record of a band, relative to the object's first
    std::vector<long> off;            // [S] first record of object s
    std::vector<double> lagbox;       // [S][K - 1][2]
    std::vector<Prior> pr;            // [S]
    std::vector<char> plain;          // [S] zeros: the launch plan's cadence classes, of which a set has one
    DevMem d_rec, d_off, d_boff, d_N, d_lagbox, d_pr;
    // per-call buffers, grown on demand: parameter vectors [cap_B][dx], results [cap_B], plan [cap_W] + [cap_W][64]
    DevMem d_theta, d_out, d_wobj, d_eidx;
    PinnedBuf<char> h_stage;          // pinned: the same four, in this order
    long cap_B = 0, cap_W = 0;
    hipStream_t stream = nullptr;
    MlogdensPlan plan;                // workspace of the launch plan, kept between calls

    size_t stage_bytes(long B, long W) const { return sizeof(double) * (size_t)B * (dx + 1) + sizeof(int) * (size_t)W * 65; }
    int ensure(long B, long W)
    {
        if (B <= cap_B && W <= cap_W) return CARMA_OK;
        const long nB = std::max(std::max(B, cap_B), 1024L), nW = std::max(std::max(W, cap_W), 64L);
        for (DevMem* b : {&d_theta, &d_out, &d_wobj, &d_eidx}) b->release();
        h_stage.release();
        cap_B = cap_W = 0;
        hipError_t e = d_theta.alloc(sizeof(double) * (size_t)nB * dx);
        if (e == hipSuccess) e = d_out.alloc(sizeof(double) * (size_t)nB);
        if (e == hipSuccess) e = d_wobj.alloc(sizeof(int) * (size_t)nW);
        if (e == hipSuccess) e = d_eidx.alloc(sizeof(int) * (size_t)nW * 64);
        if (e == hipSuccess) e = h_stage.alloc(stage_bytes(nB, nW));
        if (e != hipSuccess) return hip_fail(e, "carma_bandset_logdensity_batch: buffers");
        cap_B = nB;
        cap_W = nW;
        return CARMA_OK;
    }
};

// dynamic LDS of a workgroup, as k_logdens_carma_mband carves it: tables, work arrays, band offsets (padded to 16 ints)
static size_t mbandset_lds_bytes(int K) { return sizeof(double) * MATH_TAB_N + MbandWork::bytes(K) + sizeof(int) * 16; }

template <int P>
__global__ __launch_bounds__(64) void k_logdens_carma_mband_ms(const double* __restrict__ theta, int dx, int q, int K,
                                                              const double4* __restrict__ rec, const long* __restrict__ off,
                                                              const int* __restrict__ boff, const int* __restrict__ nobj,
                                                              const double* __restrict__ lagbox, const Prior* __restrict__ prs,
                                                              const int* __restrict__ wave_obj, const int* __restrict__ eval_idx,
                                                              int ignore_prior, double* __restrict__ out)
{
    // the carve of k_logdens_carma_mband: tables, [5][K][64] doubles, [K][64] ints, band offsets
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    const int lane = threadIdx.x;
    const size_t KL = (size_t)K * MBAND_LANES;
    double* s_tab = s_dyn;
    double* s_work = s_dyn + MATH_TAB_N;
    int* s_pos = reinterpret_cast<int*>(s_work + 5 * KL);
    int* s_boff = s_pos + KL;
    // wave-uniform: everything of the object derives from blockIdx.x alone.  These loads stand ahead of the barrier, where the
    // compiler can still show that nothing has written the tables: they stay scalar loads, the values in SGPRs
    const int s = wave_obj[blockIdx.x];
    const double4* orec = rec + off[s];
    const int N = nobj[s];
    const Prior pr = prs[s];
    const double* obox = lagbox + (long)s * 2 * (K - 1);
    math_tab_fill(s_tab);
    if (lane <= K) s_boff[lane] = boff[(long)s * (K + 1) + lane];
    __syncthreads();
    MbandWork wk;
    wk.y = s_work + lane;
    wk.e2 = s_work + KL + lane;
    wk.a = s_work + 2 * KL + lane;
    wk.mu = s_work + 3 * KL + lane;
    wk.lag = s_work + 4 * KL + lane;
    wk.pos = s_pos + lane;
    wk.boff = s_boff;
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
    const size_t lds = mbandset_lds_bytes(c->K);
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

template <class T>
static hipError_t to_device(DevMem& b, const std::vector<T>& v, size_t min_bytes = 0)
{
    hipError_t e = b.alloc(std::max(sizeof(T) * v.size(), min_bytes));
    if (e == hipSuccess && !v.empty()) e = hipMemcpy(b.as<void>(), v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
    return e;
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
    c->n.resize((size_t)S * K);
    c->N.assign(S, 0);
    c->off.resize(S);
    c->pr.resize(S);
    c->plain.assign(S, 0);
    std::vector<double> rec_all, rec;
    std::vector<int> boff;
    for (int s = 0; s < S; s++) {
        const long* so = offsets + (size_t)s * K;
        std::vector<std::vector<double>> ts(K), ys(K), es(K);
        for (int b = 0; b < K; b++) {
            ts[b].assign(time + so[b], time + so[b + 1]);
            ys[b].assign(y + so[b], y + so[b + 1]);
            es[b].assign(yerr + so[b], yerr + so[b + 1]);
            sort_dedup(ts[b], ys[b], es[b]);
            c->n[(size_t)s * K + b] = (int)ts[b].size();
            c->N[s] += (int)ts[b].size();
        }
        if (c->N[s] < 2) {
            set_error("carma_bandset_create: object %d: fewer than 2 data after the duplicate times of each band are dropped", s);
            delete c;
            return nullptr;
        }
        double ms = 0.0;
        if (max_stdev) {
            ms = max_stdev[s];
        } else if (so[1] - so[0] > 1) {                       // 10 sqrt(var(y, ddof=1)) of band 0 as given (BandsContext's default)
            double mean = 0.0, ss = 0.0;
            for (long k = so[0]; k < so[1]; k++) mean += y[k];
            mean /= (double)(so[1] - so[0]);
            for (long k = so[0]; k < so[1]; k++) ss += (y[k] - mean) * (y[k] - mean);
            ms = 10.0 * std::sqrt(ss / (double)(so[1] - so[0] - 1));
        }
        c->pr[s].measerr_dof = 50.0;   // src/include/carpack.hpp:63
        set_prior_bounds(c->pr[s], ts[0].data(), c->n[(size_t)s * K], ms);
        for (int b = 0; b + 1 < K; b++) {
            c->lagbox.push_back(lag_lo[(size_t)s * (K - 1) + b]);
            c->lagbox.push_back(lag_hi[(size_t)s * (K - 1) + b]);
        }
        mband_pack(ts, ys, es, rec, boff);                    // (its own t0: the earliest time of THIS object's bands)
        c->off[s] = (long)(rec_all.size() / 4);
        rec_all.insert(rec_all.end(), rec.begin(), rec.end());
        c->boff.insert(c->boff.end(), boff.begin(), boff.end());
    }
    if (select_device(device) != CARMA_OK) {
        delete c;
        return nullptr;
    }
    hipError_t e = to_device(c->d_rec, rec_all);
    if (e == hipSuccess) e = to_device(c->d_off, c->off);
    if (e == hipSuccess) e = to_device(c->d_boff, c->boff);
    if (e == hipSuccess) e = to_device(c->d_N, c->N);
    if (e == hipSuccess) e = to_device(c->d_lagbox, c->lagbox, sizeof(double) * 2);   // (K = 1: no boxes, never read)
    if (e == hipSuccess) e = to_device(c->d_pr, c->pr);
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
    return c->n[(size_t)s * c->K + b];
}

int carma_bandset_get_prior(const carma_bandset* h, int s, double* out3)
{
    if (!h || !out3 || s < 0 || s >= reinterpret_cast<const BSctx*>(h)->S) return CARMA_EINVAL;
    const Prior& pr = reinterpret_cast<const BSctx*>(h)->pr[s];
    out3[0] = pr.max_stdev;
    out3[1] = pr.max_freq;
    out3[2] = pr.min_freq;
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
    const int S = c->S, dx = c->dx;
    // launch plan (carma_mseries_plan.h), in the context's workspace: the waves are counted first, they size the staging block
    MlogdensPlan& pl = c->plan;
    const long bad = mlogdens_plan_count(object, B, S, c->N.data(), c->plain.data(), pl);
    if (bad >= 0) {
        set_error("carma_bandset_logdensity_batch: object[%ld] = %d out of range (nobjects = %d)", bad, object[bad], S);
        return CARMA_EINVAL;
    }
    const long W = pl.W;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    int rc = c->ensure(B, W);
    if (rc != CARMA_OK) return rc;
    double* h_th = reinterpret_cast<double*>(c->h_stage.get());
    double* h_out = h_th + (size_t)c->cap_B * dx;
    int* h_wobj = reinterpret_cast<int*>(h_out + c->cap_B);
    int* h_eidx = h_wobj + c->cap_W;
    std::memcpy(h_th, theta, sizeof(double) * (size_t)B * dx);
    mlogdens_plan_fill(pl, h_wobj, h_eidx);                   // straight into the pinned block
    hipStream_t st = c->stream;
    double *d_theta = c->d_theta.as<double>(), *d_out = c->d_out.as<double>();
    int *d_wobj = c->d_wobj.as<int>(), *d_eidx = c->d_eidx.as<int>();
    e = hipMemcpyAsync(d_theta, h_th, sizeof(double) * (size_t)B * dx, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_wobj, h_wobj, sizeof(int) * (size_t)W, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_eidx, h_eidx, sizeof(int) * (size_t)W * 64, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        (void)hipGetLastError();   // HIP's last-error is sticky: drop anything left by earlier calls
        e = launch_logdens_mband_ms(c, d_theta, d_wobj, d_eidx, W, ignore_prior, d_out, st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_out, d_out, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, st);
    // (also after a failure: the enqueued copies read and write the pinned block)
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return hip_fail(e, "carma_bandset_logdensity_batch");
    std::memcpy(out, h_out, sizeof(double) * (size_t)B);
    return CARMA_OK;
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
    if (fixed_lag)
        for (long i = 0; i < (long)B * (K - 1); i++)
            if (!std::isfinite(fixed_lag[i])) {
                set_error("carma_bandset_mle_batched: fixed_lag of start %ld, band %ld is not finite", i / (K - 1), i % (K - 1) + 1);
                return CARMA_EINVAL;
            }
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> lo, hi;
    fill_box(lo_in, (size_t)B * dx, -inf, lo);
    fill_box(hi_in, (size_t)B * dx, inf, hi);
    int band = 0;                                             // a lag never leaves its object's box, with or without the prior
    const long empty = mbandset_cut_boxes(lo.data(), hi.data(), object, B, d, K, c->lagbox.data(), fixed_lag != nullptr, &band);
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
