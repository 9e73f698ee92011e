// carma_mband_smooth.hip -- carma_bands_smooth: the interpolated light curve of one band of a multi-band fit, one parameter
// vector per lane, in one forward and one backward pass (carma_mband_smooth.h).
//
// A launch is ceil(rows / 64) workgroups of one wave, as k_logdens_carma_mband; each lane merges the bands and the requested times
// in the order ITS lags give, so vectors with different lags share a launch.  Two kernels, so that each pass has its own register
// budget:
//   k_smooth_mband_fwd<P>   the filter over the N + M points, a record per point into the scratch [wave][point][field][64]
//   k_smooth_mband_bwd<P>   the adjoint recursion back over the records; mean and variance into the caller's slots
// A lane reads only the records it wrote, the kernels follow each other on one stream.  Pad lanes repeat the wave's first row into
// scratch slots of their own and write no output.  The rows of a call are cut into chunks that reuse one scratch buffer
// (carma_mband_smooth_plan.h; carma_tune_set "MBAND_SMOOTH_CHUNK_ROWS"); a row's result depends on nothing but the row.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/carma_mi355.h"
#include "grp_device.h"
#include "carma_core.h"
#include "carma_lane.h"
#include "carma_mband.h"
#include "carma_mband_smooth.h"
#include "carma_host.h"
#include "carma_mband_ctx.h"
#include "carma_mband_smooth_plan.h"

namespace carma {

// theta = [rows][dx]; req = [M + 1] records of the requested times; sc: the chunk's scratch
template <int P>
__global__ __launch_bounds__(64) void k_smooth_mband_fwd(const double* __restrict__ theta, int dx, int q, int K, int N, int M, int bo,
                                                        const double4* __restrict__ rec, const int* __restrict__ boff,
                                                        const double4* __restrict__ req, int rows, double* __restrict__ sc, long fs,
                                                        long ps, size_t ws)
{
    static_assert(mband_smooth_fields<P>() == 2 * P + P / 2 + 5, "record layout");
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];   // all LDS is dynamic (mband_lds_bytes of K + 1 streams)
    const int lane = threadIdx.x;
    MbandWork wk;
    const double* s_tab = mband_lds_carve(s_dyn, K + 1, K, lane, boff, 0, wk);
    long e = (long)blockIdx.x * 64 + lane;
    if (e >= rows) e = (long)blockIdx.x * 64;                 // pad lanes walk the wave's first row, into slots of their own
    MbandSmoothLane<P> s;
    mband_smooth_setup<P>(theta + e * dx, q, K, bo, s, &wk);
    bool anyreal = false;
#pragma unroll
    for (int i = 0; i < P / 2; i++) anyreal = anyreal || s.m.realpair[i];
    double* mysc = sc + (size_t)blockIdx.x * ws + lane;        // [wave][point][field][64]: the strides of mband_smooth_strides
    lane_smooth_forward_mband<P>(s.m, lane_any(anyreal), s_tab, rec, req, K, N, M, wk, mysc, fs, ps);
}

// mean / var = [rows][M] in the caller's order of the times; invalid = [rows]
template <int P>
__global__ __launch_bounds__(64) void k_smooth_mband_bwd(const double* __restrict__ theta, int dx, int q, int K, int N, int M, int bo,
                                                        int rows, const double* __restrict__ sc, long fs, long ps, size_t ws,
                                                        double* __restrict__ mean, double* __restrict__ var,
                                                        int* __restrict__ invalid)
{
    const int lane = threadIdx.x;
    long e = (long)blockIdx.x * 64 + lane;
    const bool live = e < rows;
    if (!live) e = (long)blockIdx.x * 64;
    MbandSmoothLane<P> s;
    mband_smooth_setup<P>(theta + e * dx, q, K, bo, s, nullptr);
    const double* mysc = sc + (size_t)blockIdx.x * ws + lane;
    lane_smooth_backward_mband<P>(s.m, s.a_o, s.mu_o, !s.ok, N + M, mysc, fs, ps, M, live ? mean + e * (long)M : nullptr,
                                  live ? var + e * (long)M : nullptr);
    if (live) invalid[e] = s.ok ? 0 : 1;
}

struct MbandSmoothArgs {
    const double* theta;
    int dx, q, K, N, M, bo, rows;
    const double4 *rec, *req;
    const int* boff;
    double *sc, *mean, *var;
    int* invalid;
    MbandSmoothStrides sd;
};

static hipError_t launch_smooth_mband(int p, const MbandSmoothArgs& a, hipStream_t st)
{
    const dim3 grid((unsigned)((a.rows + 63) / 64)), block(64);
    const size_t lds = mband_lds_bytes(a.K + 1);               // the requested times are stream K
    auto go = [&](auto P) {
        constexpr int PP = decltype(P)::value;
        static_assert(mband_smooth_fields<PP>() == mband_smooth_nfields(PP), "carma_mband_smooth.h and its planner disagree on the record");
        hipLaunchKernelGGL((k_smooth_mband_fwd<PP>), grid, block, lds, st, a.theta, a.dx, a.q, a.K, a.N, a.M, a.bo, a.rec, a.boff, a.req,
                           a.rows, a.sc, a.sd.fs, a.sd.ps, a.sd.ws);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((k_smooth_mband_bwd<PP>), grid, block, 0, st, a.theta, a.dx, a.q, a.K, a.N, a.M, a.bo, a.rows, a.sc, a.sd.fs,
                           a.sd.ps, a.sd.ws, a.mean, a.var, a.invalid);
        return hipGetLastError();
    };
    if (p == 1) return go(std::integral_constant<int, 1>{});   // (for_order starts at 2: CAR(1) is the generic body at P = 1 here)
    return for_order(p, hipErrorInvalidValue, go);
}

}  // namespace carma

using namespace carma;

extern "C" int carma_bands_smooth(carma_bands* h, const double* theta, int B, int band, const double* tout, int M, double* mean,
                                  double* var, double* band_mean, double* band_var, int* invalid)
{
    static const char* const who = "carma_bands_smooth";
    Bctx* c = reinterpret_cast<Bctx*>(h);
    const std::string bad = mband_smooth_check(h != nullptr, c ? c->K : 0, c ? c->o.N : 0, theta, B, band, tout, M, mean, var, band_mean,
                                               band_var);
    if (!bad.empty()) {
        set_error("%s: %s", who, bad.c_str());
        return CARMA_EINVAL;
    }
    const int ng = c->o.N + M;
    const MbandSmoothTimes tm = mband_smooth_times(tout, M, c->o.t0);
    const long forced = tune_get(TUNE_MBAND_SMOOTH_CHUNK_ROWS);
    const MbandSmoothChunks ch = mband_smooth_chunks(c->p, ng, B, forced == TUNE_UNSET ? 0 : forced);
    const MbandSmoothStrides sd = mband_smooth_strides(c->p, ng);

    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    (void)hipGetLastError();   // HIP's last-error is sticky: drop anything left by earlier calls
    DevMem b_theta, b_req, b_sc, b_mean, b_var, b_inv, b_band;
    std::vector<int> inv((size_t)B, 0);
    e = b_theta.alloc(sizeof(double) * (size_t)B * c->dx);
    if (e == hipSuccess) e = b_req.alloc(sizeof(double) * tm.rec.size());
    if (e == hipSuccess) e = b_sc.alloc(sizeof(double) * (size_t)ch.waves * sd.ws);
    if (e == hipSuccess) e = b_mean.alloc(sizeof(double) * (size_t)B * M);
    if (e == hipSuccess) e = b_var.alloc(sizeof(double) * (size_t)B * M);
    if (e == hipSuccess) e = b_inv.alloc(sizeof(int) * (size_t)B);
    if (e == hipSuccess && band_mean) e = b_band.alloc(sizeof(double) * 2 * (size_t)M);
    if (e != hipSuccess) return hip_fail(e, "carma_bands_smooth: allocation");
    hipStream_t st = c->stream;
    e = hipMemcpyAsync(b_theta.as<void>(), theta, sizeof(double) * (size_t)B * c->dx, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(b_req.as<void>(), tm.rec.data(), sizeof(double) * tm.rec.size(), hipMemcpyHostToDevice, st);
    for (long r0 = 0; r0 < B && e == hipSuccess; r0 += ch.rows) {
        MbandSmoothArgs a{};
        a.theta = b_theta.as<double>() + (size_t)r0 * c->dx;
        a.dx = c->dx;
        a.q = c->q;
        a.K = c->K;
        a.N = c->o.N;
        a.M = M;
        a.bo = band;
        a.rows = (int)std::min<long>(ch.rows, B - r0);
        a.rec = c->d_rec.as<const double4>();
        a.req = b_req.as<const double4>();
        a.boff = c->d_boff.as<const int>();
        a.sc = b_sc.as<double>();
        a.mean = b_mean.as<double>() + (size_t)r0 * M;
        a.var = b_var.as<double>() + (size_t)r0 * M;
        a.invalid = b_inv.as<int>() + r0;
        a.sd = sd;
        e = launch_smooth_mband(c->p, a, st);
    }
    double* d_band = b_band.as<double>();
    if (e == hipSuccess && band_mean)
        e = launch_smooth_band(b_mean.as<double>(), b_var.as<double>(), b_inv.as<int>(), B, M, d_band, d_band + M, st);
    if (e == hipSuccess && mean) e = hipMemcpyAsync(mean, b_mean.as<void>(), sizeof(double) * (size_t)B * M, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && var) e = hipMemcpyAsync(var, b_var.as<void>(), sizeof(double) * (size_t)B * M, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && band_mean) e = hipMemcpyAsync(band_mean, d_band, sizeof(double) * M, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && band_mean) e = hipMemcpyAsync(band_var, d_band + M, sizeof(double) * M, hipMemcpyDeviceToHost, st);
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
