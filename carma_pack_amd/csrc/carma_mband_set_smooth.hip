// carma_mband_set_smooth.hip -- carma_bandset_smooth: the interpolated light curves of MANY multi-band objects in one call: the two
// passes of carma_mband_smooth.hip with the JOB chosen per wave from tables, the way k_logdens_carma_mband_ms chooses the object
// (DESIGN.md section 3, K1mb-set-s).
//
// A job is (object s, output band bo, one list of requested times): what the walk of a wave is uniform in -- the record base, the
// band offsets in LDS, N = nobj[s], M, bo, the job's request records and the wave's scratch base all derive from blockIdx.x alone.
//   k_smooth_mband_fwd_ms<P>   the filter over the N_s + M points of the wave's job, a record per point into the wave's scratch
//   k_smooth_mband_bwd_ms<P>   the adjoint recursion back over the records; mean and variance into the caller's ragged slots
// Lane l of wave w works on the caller's row row_idx[64 w + l]; pad lanes (-1; they only trail, lane 0 is live) repeat the wave's
// first row into scratch slots of their own and write no output.  The bodies are mband_smooth_setup, lane_smooth_forward_mband
// and lane_smooth_backward_mband UNCHANGED: a row has the bits carma_bands_smooth gives for it on a handle of its object alone.
// Scratch is [wave][point][field][64] as there, but ng = N_s + M differs from wave to wave, so a wave's base comes from a table
// (wave_sc, doubles); consecutive waves are cut into chunks that reuse one buffer (carma_mband_set_smooth_plan.h; carma_tune_set
// "MBANDSET_SMOOTH_CHUNK_WAVES").  The cost of the design: a wave never mixes jobs, so ONE row per (object, band) occupies a wave
// of which 63 lanes are pads.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/carma_mi355.h"
#include "grp_device.h"
#include "carma_core.h"
#include "carma_lane.h"
#include "carma_mband.h"
#include "carma_mband_smooth.h"
#include "carma_host.h"
#include "carma_mband_set_ctx.h"
#include "carma_mband_set_smooth_plan.h"

namespace carma {

// theta = [B][dx]; rec / off / boff / nobj: the set's records and tables; req: the jobs' request records; the wave tables start at
// the chunk's first wave; sc: the chunk's scratch
template <int P>
__global__ __launch_bounds__(64) void k_smooth_mband_fwd_ms(const double* __restrict__ theta, int dx, int q, int K,
                                                           const double4* __restrict__ rec, const long* __restrict__ off,
                                                           const int* __restrict__ boff, const int* __restrict__ nobj,
                                                           const double4* __restrict__ req, const int* __restrict__ wave_job,
                                                           const int* __restrict__ job_obj, const int* __restrict__ job_band,
                                                           const int* __restrict__ job_M, const long* __restrict__ job_req,
                                                           const int* __restrict__ row_idx, const long* __restrict__ wave_sc,
                                                           double* __restrict__ sc, long fs, long ps)
{
    static_assert(mband_smooth_fields<P>() == 2 * P + P / 2 + 5, "record layout");
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];   // all LDS is dynamic (mband_lds_bytes of K + 1 streams)
    const int lane = threadIdx.x;
    // wave-uniform: everything of the job derives from blockIdx.x alone.  These loads stand ahead of the carve and its barrier,
    // where the compiler can still show that nothing has written the tables: they stay scalar loads, the values in SGPRs
    const int job = wave_job[blockIdx.x];
    const int s = job_obj[job];
    const double4* orec = rec + off[s];
    const int N = nobj[s], M = job_M[job], bo = job_band[job];
    const double4* jreq = req + job_req[job];
    double* wsc = sc + wave_sc[blockIdx.x];
    MbandWork wk;
    const double* s_tab = mband_lds_carve(s_dyn, K + 1, K, lane, boff, s, wk);
    const int* rw = row_idx + (long)blockIdx.x * 64;
    long e = rw[lane];
    if (e < 0) e = rw[0];                                     // pad lanes walk the wave's first row, into slots of their own
    MbandSmoothLane<P> sl;
    mband_smooth_setup<P>(theta + e * dx, q, K, bo, sl, &wk);
    bool anyreal = false;
#pragma unroll
    for (int i = 0; i < P / 2; i++) anyreal = anyreal || sl.m.realpair[i];
    lane_smooth_forward_mband<P>(sl.m, lane_any(anyreal), s_tab, orec, jreq, K, N, M, wk, wsc + lane, fs, ps);
}

// mean / var: the caller's ragged outputs, row i from out_off[i]; invalid = [B]
template <int P>
__global__ __launch_bounds__(64) void k_smooth_mband_bwd_ms(const double* __restrict__ theta, int dx, int q, int K,
                                                           const int* __restrict__ nobj, const int* __restrict__ wave_job,
                                                           const int* __restrict__ job_obj, const int* __restrict__ job_band,
                                                           const int* __restrict__ job_M, const int* __restrict__ row_idx,
                                                           const long* __restrict__ wave_sc, const long* __restrict__ out_off,
                                                           const double* __restrict__ sc, long fs, long ps,
                                                           double* __restrict__ mean, double* __restrict__ var,
                                                           int* __restrict__ invalid)
{
    const int lane = threadIdx.x;
    const int job = wave_job[blockIdx.x];
    const int N = nobj[job_obj[job]], M = job_M[job], bo = job_band[job];
    const double* wsc = sc + wave_sc[blockIdx.x];
    const int* rw = row_idx + (long)blockIdx.x * 64;
    long e = rw[lane];
    const bool live = e >= 0;
    if (!live) e = rw[0];
    MbandSmoothLane<P> sl;
    mband_smooth_setup<P>(theta + e * dx, q, K, bo, sl, nullptr);
    const long oo = out_off[e];
    lane_smooth_backward_mband<P>(sl.m, sl.a_o, sl.mu_o, !sl.ok, N + M, wsc + lane, fs, ps, M, live ? mean + oo : nullptr,
                                  live ? var + oo : nullptr);
    if (live) invalid[e] = sl.ok ? 0 : 1;
}

// the device side of a call: the tables are those of MbandSetSmoothPlan, the wave tables whole (a chunk starts at w0)
struct MbandSetSmoothArgs {
    const double* theta;
    const double4* req;
    const int *wave_job, *job_obj, *job_band, *job_M, *row_idx;
    const long *job_req, *wave_sc, *out_off;
    double *sc, *mean, *var;
    int* invalid;
    MbandSmoothStrides sd;
};

// waves [w0, w1) of the plan: both passes
static hipError_t launch_smooth_mband_ms(const BSctx* c, const MbandSetSmoothArgs& a, long w0, long w1, hipStream_t st)
{
    if (w1 <= w0) return hipSuccess;
    const dim3 grid((unsigned)(w1 - w0)), block(64);
    const size_t lds = mband_lds_bytes(c->K + 1);              // the requested times are stream K
    auto go = [&](auto P) {
        constexpr int PP = decltype(P)::value;
        static_assert(mband_smooth_fields<PP>() == mband_smooth_nfields(PP), "carma_mband_smooth.h and its planner disagree on the record");
        hipLaunchKernelGGL((k_smooth_mband_fwd_ms<PP>), grid, block, lds, st, a.theta, c->dx, c->q, c->K, c->d_rec.as<const double4>(),
                           c->d_off.as<const long>(), c->d_boff.as<const int>(), c->d_N.as<const int>(), a.req, a.wave_job + w0,
                           a.job_obj, a.job_band, a.job_M, a.job_req, a.row_idx + w0 * 64, a.wave_sc + w0, a.sc, a.sd.fs, a.sd.ps);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((k_smooth_mband_bwd_ms<PP>), grid, block, 0, st, a.theta, c->dx, c->q, c->K, c->d_N.as<const int>(),
                           a.wave_job + w0, a.job_obj, a.job_band, a.job_M, a.row_idx + w0 * 64, a.wave_sc + w0, a.out_off, a.sc,
                           a.sd.fs, a.sd.ps, a.mean, a.var, a.invalid);
        return hipGetLastError();
    };
    if (c->p == 1) return go(std::integral_constant<int, 1>{});   // (for_order starts at 2: CAR(1) is the generic body at P = 1 here)
    return for_order(c->p, hipErrorInvalidValue, go);
}

}  // namespace carma

using namespace carma;

extern "C" int carma_bandset_smooth(carma_bandset* h, const double* theta, const int* object, const int* band, int B,
                                    const double* tout, const long* toff, double* mean, double* var, int* invalid)
{
    static const char* const who = "carma_bandset_smooth";
    BSctx* c = reinterpret_cast<BSctx*>(h);
    const std::string bad = mbandset_smooth_check(h != nullptr, c ? c->S : 0, c ? c->K : 0, c ? c->m.N.data() : nullptr, theta, object,
                                                  band, B, tout, toff, mean, var);
    if (!bad.empty()) {
        set_error("%s: %s", who, bad.c_str());
        return CARMA_EINVAL;
    }
    const long forced = tune_get(TUNE_MBANDSET_SMOOTH_CHUNK_WAVES);
    const MbandSetSmoothPlan pl = mbandset_smooth_plan(c->p, object, band, B, tout, toff, c->m.N.data(), c->m.t0.data(),
                                                       forced == TUNE_UNSET ? 0 : forced);
    const size_t T = (size_t)(toff[B] - toff[0]);
    const size_t W = (size_t)pl.W, J = (size_t)pl.J;
    // the tables side by side, one copy each: ints wave_job [W], job_obj, job_band, job_M [J], row_idx [64 W]; longs job_req [J],
    // wave_sc [W], out_off [B]
    std::vector<int> ti;
    ti.reserve(65 * W + 3 * J);
    for (const std::vector<int>* v : {&pl.wave_job, &pl.job_obj, &pl.job_band, &pl.job_M, &pl.row_idx}) ti.insert(ti.end(), v->begin(), v->end());
    std::vector<long> tl;
    tl.reserve(J + W + (size_t)B);
    for (const std::vector<long>* v : {&pl.job_req, &pl.wave_sc, &pl.out_off}) tl.insert(tl.end(), v->begin(), v->end());

    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    (void)hipGetLastError();   // HIP's last-error is sticky: drop anything left by earlier calls
    DevMem b_theta, b_req, b_ti, b_tl, b_sc, b_mean, b_var, b_inv;
    std::vector<int> inv((size_t)B, 0);
    e = b_theta.alloc(sizeof(double) * (size_t)B * c->dx);
    if (e == hipSuccess) e = b_req.alloc(sizeof(double) * pl.req.size());
    if (e == hipSuccess) e = b_ti.alloc(sizeof(int) * ti.size());
    if (e == hipSuccess) e = b_tl.alloc(sizeof(long) * tl.size());
    if (e == hipSuccess) e = b_sc.alloc(sizeof(double) * pl.sc_max);
    if (e == hipSuccess) e = b_mean.alloc(sizeof(double) * T);
    if (e == hipSuccess) e = b_var.alloc(sizeof(double) * T);
    if (e == hipSuccess) e = b_inv.alloc(sizeof(int) * (size_t)B);
    if (e != hipSuccess) return hip_fail(e, "carma_bandset_smooth: allocation");
    hipStream_t st = c->stream;
    e = hipMemcpyAsync(b_theta.as<void>(), theta, sizeof(double) * (size_t)B * c->dx, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(b_req.as<void>(), pl.req.data(), sizeof(double) * pl.req.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(b_ti.as<void>(), ti.data(), sizeof(int) * ti.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(b_tl.as<void>(), tl.data(), sizeof(long) * tl.size(), hipMemcpyHostToDevice, st);
    MbandSetSmoothArgs a{};
    a.theta = b_theta.as<double>();
    a.req = b_req.as<const double4>();
    a.wave_job = b_ti.as<const int>();
    a.job_obj = a.wave_job + W;
    a.job_band = a.job_obj + J;
    a.job_M = a.job_band + J;
    a.row_idx = a.job_M + J;
    a.job_req = b_tl.as<const long>();
    a.wave_sc = a.job_req + J;
    a.out_off = a.wave_sc + W;
    a.sc = b_sc.as<double>();
    a.mean = b_mean.as<double>();
    a.var = b_var.as<double>();
    a.invalid = b_inv.as<int>();
    a.sd = mband_smooth_strides(c->p, 1);
    for (size_t k = 0; k + 1 < pl.chunk0.size() && e == hipSuccess; k++) e = launch_smooth_mband_ms(c, a, pl.chunk0[k], pl.chunk0[k + 1], st);
    if (e == hipSuccess) e = hipMemcpyAsync(mean, b_mean.as<void>(), sizeof(double) * T, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(var, b_var.as<void>(), sizeof(double) * T, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(inv.data(), b_inv.as<void>(), sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, st);
    // (also after a failure: the enqueued copies read and write the caller's arrays)
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return hip_fail(e, who);
    bool any = false;
    for (int i = 0; i < B; i++) {
        any |= inv[i] != 0;
        if (invalid) invalid[i] = inv[i];
    }
    return (any && !invalid) ? 1 : CARMA_OK;
}
