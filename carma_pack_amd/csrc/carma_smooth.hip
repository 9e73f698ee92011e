// carma_smooth.hip -- the interpolated light curve and its posterior band in one pass (carma_smooth_carma /
// carma_smooth_car1).
//
// carma_predict_* filters the whole series again for every requested time: O(M n p^2) for M times on n data.  Here the
// fixed-interval smoother of carma_smooth.h walks the merged grid of data and requested times once forward and once backward,
// O((n + M) p^2), for K models at once -- one lane group per model (CAR(1): one lane), every model on the same series and grid,
// so the loop of a wave is uniform:
//   k_smooth_carma<P,G>  forward pass into the scratch records, a workgroup barrier (a workgroup is one wave), backward pass
//   k_smooth_car1        the scalar recursion, one lane per model
//   k_smooth_band        the moment-matched mixture of the K predictive distributions per time, on the device
// Groups past the last model of a launch repeat it (into scratch slots of their own) and store no output.  A model's
// outputs depend on nothing but the model, the series and the grid: not on its neighbours, not on how the call is cut into
// chunks (carma_tune_set "SMOOTH_CHUNK_MODELS").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/carma_mi355.h"
#include "grp_device.h"
#include "carma_core.h"
#include "carma_host.h"
#include "carma_smooth.h"
#include "carma_smooth_plan.h"

namespace carma {

// par = [kc][3 P + 2] (roots, MA coefficients, sigsqr, mu); rec / grp: the chunk's scratch (carma_smooth_plan.h);
// mean / var = [kc][M], singular = [kc]
template <int P, int G>
__global__ __launch_bounds__(64) void k_smooth_carma(const double* __restrict__ par, int kc, const double4* __restrict__ series,
                                                     const double* __restrict__ grid, const int* __restrict__ src, int ng, int M,
                                                     double4* __restrict__ rec, double4* __restrict__ grp,
                                                     double* __restrict__ mean, double* __restrict__ var,
                                                     int* __restrict__ singular)
{
    __shared__ double4 xch[64];
    __shared__ double2 xch2[64];
    constexpr int E = 64 / G;
    const int tid = threadIdx.x;
    Grp<G> g{xch, tid & 63, xch2};
    const int e = tid / G;
    long k = (long)blockIdx.x * E + e;
    const bool live = k < kc;
    if (!live) k = kc - 1;
    const double* pm = par + k * (3 * P + 2);
    Model<P> m;
    model_from_roots<P, G>(g, pm, pm + 2 * P, pm[3 * P], m);
    const double mu = pm[3 * P + 1];
    FilterConsts<P> fc;
    filter_reset<P, G>(g, m, fc);
    double4* myrec = rec + (size_t)blockIdx.x * ng * 64 + tid;
    double4* mygrp = grp + (size_t)blockIdx.x * ng * E + e;
    smooth_forward<P, G>(g, m, fc, series, grid, src, ng, mu, myrec, 64, mygrp, E);
    __syncthreads();                                          // lane 0 wrote the group records, every lane of the group reads them
    smooth_backward<P, G>(g, fc, src, ng, mu, myrec, 64, mygrp, E, live ? mean + k * (long)M : nullptr,
                          live ? var + k * (long)M : nullptr);
    if (live && g.lane() == 0) singular[k] = fc.sing ? 1 : 0;
}

// CAR(1): par = [kc][3] (sigsqr, omega, mu); sc: five planes of ng x lanes doubles, lanes = 64 gridDim.x
__global__ __launch_bounds__(64) void k_smooth_car1(const double* __restrict__ par, int kc, const double4* __restrict__ series,
                                                    const double* __restrict__ grid, const int* __restrict__ src, int ng, int M,
                                                    double* __restrict__ sc, double* __restrict__ mean, double* __restrict__ var)
{
    const long L = (long)blockIdx.x * 64 + threadIdx.x;
    const long lanes = (long)gridDim.x * 64;
    const bool live = L < kc;
    const long k = live ? L : kc - 1;
    const double* pm = par + 3 * k;
    smooth_car1(pm[0], pm[1], pm[2], series, grid, src, ng, sc + L, lanes, lanes * ng, live ? mean + k * (long)M : nullptr,
                live ? var + k * (long)M : nullptr);
}

// band[i] = moments of the equal-weight mixture of the models that are not singular: two passes in ascending k, one thread per
// time, no atomics.  No such model: 0 / 0.
__global__ __launch_bounds__(64) void k_smooth_band(const double* __restrict__ mean, const double* __restrict__ var,
                                                    const int* __restrict__ singular, int K, int M, double* __restrict__ bmean,
                                                    double* __restrict__ bvar)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= M) return;
    double sm = 0.0;
    int kk = 0;
    for (int k = 0; k < K; k++) {
        if (singular[k]) continue;
        sm += mean[(long)k * M + i];
        kk++;
    }
    const double mb = sm / (double)kk;
    double sv = 0.0;
    for (int k = 0; k < K; k++) {
        if (singular[k]) continue;
        const double d = mean[(long)k * M + i] - mb;
        sv += var[(long)k * M + i] + d * d;
    }
    bmean[i] = mb;
    bvar[i] = sv / (double)kk;
}

// (declared in carma_launch.h: carma_bands_smooth mixes its rows with the same kernel)
hipError_t launch_smooth_band(const double* mean, const double* var, const int* singular, int K, int M, double* bmean, double* bvar,
                              hipStream_t st)
{
    hipLaunchKernelGGL(k_smooth_band, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, st, mean, var, singular, K, M, bmean, bvar);
    return hipGetLastError();
}

struct SmoothArgs {
    const double* par;
    int kc;
    const double4* series;
    const double* grid;
    const int* src;
    int ng, M;
    double4 *rec, *grp;
    double *mean, *var;
    int* singular;
};

template <int P>
static hipError_t launch_smooth_p(const SmoothArgs& a)
{
    constexpr int G = GroupOf<P>::value;
    constexpr int E = 64 / G;
    hipLaunchKernelGGL((k_smooth_carma<P, G>), dim3((unsigned)((a.kc + E - 1) / E)), dim3(64), 0, nullptr, a.par, a.kc, a.series,
                       a.grid, a.src, a.ng, a.M, a.rec, a.grp, a.mean, a.var, a.singular);
    return hipGetLastError();
}

static hipError_t launch_smooth(int p, const SmoothArgs& a)
{
    (void)hipGetLastError();   // HIP's last-error is sticky: drop anything left by earlier calls
    if (p == 1) {
        hipLaunchKernelGGL(k_smooth_car1, dim3((unsigned)((a.kc + 63) / 64)), dim3(64), 0, nullptr, a.par, a.kc, a.series, a.grid,
                           a.src, a.ng, a.M, reinterpret_cast<double*>(a.rec), a.mean, a.var);
        return hipGetLastError();
    }
    return for_order(p, hipErrorInvalidValue, [&](auto P) { return launch_smooth_p<decltype(P)::value>(a); });
}

// par = [K][pw] rows as the kernels read them (validated, roots normalised); p == 1: pw = 3
static int smooth_host(const char* who, const double* time, const double* y, const double* yerr, int n, int p, int K,
                       const std::vector<double>& par, const double* tout, int M, double* mean, double* var, double* bmean,
                       double* bvar, int* singular, int* n_out, int device)
{
    for (int i = 0; i < M; i++) {
        if (!std::isfinite(tout[i])) {
            set_error("%s: tout[%d] is not finite", who, i);
            return CARMA_EINVAL;
        }
    }
    DevMem b_s, b_grid, b_src, b_par, b_sing, b_rec, b_grp, b_mean, b_var, b_band;
    std::vector<double> t(time, time + n), yy(y, y + n), ee(yerr, yerr + n);
    sort_dedup(t, yy, ee);
    const int m = (int)t.size();
    if (n_out) *n_out = m;
    const int rc = select_device(device);
    if (rc != CARMA_OK) return rc;
    const SmoothGrid sg = smooth_merge(t.data(), m, tout, M);
    const std::vector<double> s = pack_series(t, yy, ee);
    const int pw = (int)(par.size() / (size_t)K);
    const int G = p > 1 ? group_of(p) : 0;
    const long forced = tune_get(TUNE_SMOOTH_CHUNK_MODELS);
    const SmoothChunks ch = smooth_chunks(G, sg.ng, K, forced == TUNE_UNSET ? 0 : forced);

    hipError_t e = b_s.alloc(sizeof(double) * s.size());
    if (e == hipSuccess) e = b_grid.alloc(sizeof(double) * sg.ng);
    if (e == hipSuccess) e = b_src.alloc(sizeof(int) * sg.ng);
    if (e == hipSuccess) e = b_par.alloc(sizeof(double) * par.size());
    if (e == hipSuccess) e = b_sing.alloc(sizeof(int) * K);
    if (e == hipSuccess) e = b_rec.alloc((G ? 32 : 8) * ch.rec_elems);
    if (e == hipSuccess && G) e = b_grp.alloc(32 * ch.grp_elems);
    if (e == hipSuccess) e = b_mean.alloc(sizeof(double) * (size_t)K * M);
    if (e == hipSuccess) e = b_var.alloc(sizeof(double) * (size_t)K * M);
    if (e == hipSuccess && bmean) e = b_band.alloc(sizeof(double) * 2 * (size_t)M);
    double *d_s = b_s.as<double>(), *d_grid = b_grid.as<double>(), *d_par = b_par.as<double>(), *d_mean = b_mean.as<double>(),
           *d_var = b_var.as<double>(), *d_band = b_band.as<double>();
    int *d_src = b_src.as<int>(), *d_sing = b_sing.as<int>();
    if (e == hipSuccess) e = hipMemcpy(d_s, s.data(), sizeof(double) * s.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_grid, sg.grid.data(), sizeof(double) * sg.ng, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_src, sg.src.data(), sizeof(int) * sg.ng, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_sing, 0, sizeof(int) * K);
    for (long k0 = 0; k0 < K && e == hipSuccess; k0 += ch.models) {
        SmoothArgs a{};
        a.par = d_par + (size_t)k0 * pw;
        a.kc = (int)std::min<long>(ch.models, K - k0);
        a.series = reinterpret_cast<const double4*>(d_s);
        a.grid = d_grid;
        a.src = d_src;
        a.ng = sg.ng;
        a.M = M;
        a.rec = b_rec.as<double4>();
        a.grp = b_grp.as<double4>();
        a.mean = d_mean + (size_t)k0 * M;
        a.var = d_var + (size_t)k0 * M;
        a.singular = d_sing + k0;
        e = launch_smooth(p, a);
    }
    if (e == hipSuccess && bmean) {
        e = launch_smooth_band(d_mean, d_var, d_sing, K, M, d_band, d_band + M, nullptr);
    }
    // (blocking copies on the null stream: they wait for the launches above)
    if (e == hipSuccess && mean) e = hipMemcpy(mean, d_mean, sizeof(double) * (size_t)K * M, hipMemcpyDeviceToHost);
    if (e == hipSuccess && var) e = hipMemcpy(var, d_var, sizeof(double) * (size_t)K * M, hipMemcpyDeviceToHost);
    if (e == hipSuccess && bmean) e = hipMemcpy(bmean, d_band, sizeof(double) * M, hipMemcpyDeviceToHost);
    if (e == hipSuccess && bmean) e = hipMemcpy(bvar, d_band + M, sizeof(double) * M, hipMemcpyDeviceToHost);
    std::vector<int> sing(K, 0);
    if (e == hipSuccess) e = hipMemcpy(sing.data(), d_sing, sizeof(int) * K, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, who);
    bool any = false;
    for (int k = 0; k < K; k++) {
        any |= sing[k] != 0;
        if (singular) singular[k] = sing[k];
    }
    return (any && !singular) ? 1 : CARMA_OK;
}

// the argument checks both entry points share; 0 or CARMA_EINVAL
static int smooth_check(const char* who, const void* time, const void* y, const void* yerr, int n, int K, const void* tout, int M,
                        const double* mean, const double* var, const double* bmean, const double* bvar)
{
    if (K < 1 || M < 1) {
        set_error("%s: need nmodels >= 1 and M >= 1 (got nmodels = %d, M = %d)", who, K, M);
        return CARMA_EINVAL;
    }
    if (!time || !y || !yerr || n < 1 || !tout) {
        set_error("%s: bad argument (non-null arrays, n >= 1)", who);
        return CARMA_EINVAL;
    }
    if ((mean == nullptr) != (var == nullptr) || (bmean == nullptr) != (bvar == nullptr) || (!mean && !bmean)) {
        set_error("%s: mean and var, band_mean and band_var come in pairs, and one pair at least is needed", who);
        return CARMA_EINVAL;
    }
    return CARMA_OK;
}

}  // namespace carma

using namespace carma;

extern "C" {

int carma_smooth_carma(const double* time, const double* y, const double* yerr, int n, int p, int nmodels, const double* sigsqr,
                       const double* omega_re_im, const double* ma, int nma, const double* mu, const double* tout, int M,
                       double* mean, double* var, double* band_mean, double* band_var, int* singular, int* n_out, int device)
{
    static const char* const who = "carma_smooth_carma";
    if (smooth_check(who, time, y, yerr, n, nmodels, tout, M, mean, var, band_mean, band_var) != CARMA_OK) return CARMA_EINVAL;
    if (p < 2 || p > CARMA_PMAX || !sigsqr || !omega_re_im || !ma) {
        set_error("%s: bad argument (non-null model arrays, 2 <= p <= %d)", who, CARMA_PMAX);
        return CARMA_EINVAL;
    }
    if (nma < 1 || nma > p) {
        set_error("%s: need 1 <= nma <= p (got nma = %d, p = %d)", who, nma, p);
        return CARMA_EINVAL;
    }
    const int pw = 3 * p + 2;
    std::vector<double> par((size_t)nmodels * pw, 0.0);
    for (int k = 0; k < nmodels; k++) {
        if (!(sigsqr[k] > 0.0)) {
            set_error("%s: model %d: need sigsqr > 0", who, k);
            return CARMA_EINVAL;
        }
        if (pack_model_row(p, omega_re_im + (size_t)k * 2 * p, ma + (size_t)k * nma, nma, sigsqr[k], mu ? mu[k] : 0.0,
                           par.data() + (size_t)k * pw) != CARMA_OK) {
            set_error("%s: model %d: the AR roots must be real or come in complex-conjugate pairs", who, k);
            return CARMA_EINVAL;
        }
    }
    return smooth_host(who, time, y, yerr, n, p, nmodels, par, tout, M, mean, var, band_mean, band_var, singular, n_out, device);
}

int carma_smooth_car1(const double* time, const double* y, const double* yerr, int n, int nmodels, const double* sigsqr,
                      const double* omega, const double* mu, const double* tout, int M, double* mean, double* var,
                      double* band_mean, double* band_var, int* singular, int* n_out, int device)
{
    static const char* const who = "carma_smooth_car1";
    if (smooth_check(who, time, y, yerr, n, nmodels, tout, M, mean, var, band_mean, band_var) != CARMA_OK) return CARMA_EINVAL;
    if (!sigsqr || !omega) {
        set_error("%s: bad argument (null sigsqr or omega)", who);
        return CARMA_EINVAL;
    }
    std::vector<double> par((size_t)nmodels * 3, 0.0);
    for (int k = 0; k < nmodels; k++) {
        if (!(sigsqr[k] > 0.0) || !(omega[k] > 0.0)) {
            set_error("%s: model %d: need sigsqr > 0 and omega > 0", who, k);
            return CARMA_EINVAL;
        }
        par[3 * (size_t)k] = sigsqr[k];
        par[3 * (size_t)k + 1] = omega[k];
        par[3 * (size_t)k + 2] = mu ? mu[k] : 0.0;
    }
    return smooth_host(who, time, y, yerr, n, 1, nmodels, par, tout, M, mean, var, band_mean, band_var, singular, n_out, device);
}

}  // extern "C"
