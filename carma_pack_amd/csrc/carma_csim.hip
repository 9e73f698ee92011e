// carma_csim.hip -- CONDITIONAL simulation of many paths on one series, every path with a model of its own
// (carma_simulate_cond_carma / carma_simulate_cond_car1).
//
// What a user does with `for i in range(nsim): ysim[i] = sample.simulate(t, bestfit='random')` (the forecasting and
// interpolation plots of the reference's guide): K draws of the process at M times given the measured series, draw k with
// the parameters of one posterior sample.  Matheron's rule, as KalmanFilter*::Simulate of this package states it,
//     f*|y  =  f~*  +  E[f* | y - y~],      f~ = an unconditional path on (data times U requested times),
//                                            y~ = f~(data times) + measurement noise,
// for all K paths in TWO launches:
//   k_csim_paths_*   one lane group (CAR(1): one lane) per path: simulate_run / simulate_car1 on the merged grid with the key
//                    (seed, path0 + k), then the path's residual series  y - mu_k - y~_k  as series records of its own;
//   k_csim_predict_* one lane group (one lane) per (path, time) pair: predict_run / predict_car1 of the path's residual
//                    series at that time, added to the unconditional value there, plus mu_k.
// Both reuse the device functions of the single-model entry points unchanged, and the three places where this file adds
// numbers of its own (the residual, f~ + mean, + mu) are evaluated without contraction: a caller can rebuild every path
// bit for bit from carma_simulate_* and carma_predict_* (the optional outputs `uncond` and `noise` are what that takes).
//
// Scratch per path: n residual records (32 n bytes) and the unconditional path (8 (n + M) bytes), plus 8 n for the
// normals when the caller asks for them; paths are processed in chunks that keep it under CSIM_SCRATCH_CAP.  A chunk
// continues the keys path0 + k, so the chunk size (carma_tune_set "CSIM_CHUNK_PATHS") never changes a bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "../../include/carma_mi355.h"
#include "grp_device.h"
#include "carma_core.h"
#include "carma_host.h"
#include "carma_predict.h"
#include "carma_simulate.h"

namespace carma {

constexpr size_t CSIM_SCRATCH_CAP = (size_t)256 << 20;      // bytes of residual records + unconditional paths per chunk

// Residual of datum j for one path: (y - mu) - (f~ + yerr z), every operation rounded on its own (a host restatement
// in plain doubles gives the same bits; y - 0.0 is exact, so centred data with mu = 0 keep theirs).
CARMA_DEV double csim_resid(double y, double mu, double f, double yerr, double z)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double noise = yerr * z;
    const double ytilde = f + noise;
    const double yc = y - mu;
    return yc - ytilde;
}

// f~ + E[f* | residual]: an addition of its own (predict_car1 forms its mean as a product, which would fuse into it)
CARMA_DEV double csim_add(double f, double pm)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return f + pm;
}

// Unconditional paths and residual series of `kc` paths: one lane group per path.  par = [kc][3 P + 2] (roots, MA
// coefficients, sigsqr, mu), grid = the ng = n + M merged times, dpos[j] = position of datum j in it.
// uncond = [kc][ng], resid = [kc][n] records, noise = [kc][n] or null, singular = [kc].
template <int P, int G>
__global__ __launch_bounds__(64) void k_csim_paths_carma(const double* __restrict__ par, int kc,
                                                         const double4* __restrict__ series, const double* __restrict__ yerr,
                                                         int n, const double* __restrict__ grid, int ng,
                                                         const int* __restrict__ dpos, unsigned seed0, unsigned seed1,
                                                         unsigned path0, double* uncond, double4* __restrict__ resid,
                                                         double* __restrict__ noise, int* __restrict__ singular)
{
    __shared__ double4 xch[64];
    __shared__ double2 xch2[64];
    const int tid = threadIdx.x;
    Grp<G> g{xch, tid & 63, xch2};
    long k = ((long)blockIdx.x * 64 + tid) / G;
    const bool live = k < kc;
    if (!live) k = kc - 1;
    const double* pm = par + k * (3 * P + 2);
    Model<P> m;
    model_from_roots<P, G>(g, pm, pm + 2 * P, pm[3 * P], m);
    const double mu = pm[3 * P + 1];
    const RngKey key{seed0, seed1, path0 + (unsigned)k};
    double* f = uncond + k * (long)ng;
    bool sing;
    // (shadow groups past the end redo the last path and write the same values)
    simulate_run<P, G>(g, m, grid, ng, key, f, &sing);
    __syncthreads();                                          // lane 0 wrote the path, every lane of the group reads it
    if (live) {
        for (int j = g.lane(); j < n; j += G) {
            const double4 r = series[j];
            const double z = rng_normal(key, (uint64_t)j, 1);
            resid[k * (long)n + j] = make_double4(r.x, csim_resid(r.y, mu, f[dpos[j]], yerr[j], z), r.z, r.w);
            if (noise) noise[k * (long)n + j] = z;
        }
        if (g.lane() == 0) singular[k] = sing ? 1 : 0;
    }
}

// CAR(1): one lane per path; par = [kc][3] (sigsqr, omega, mu)
__global__ __launch_bounds__(64) void k_csim_paths_car1(const double* __restrict__ par, int kc,
                                                        const double4* __restrict__ series, const double* __restrict__ yerr,
                                                        int n, const double* __restrict__ grid, int ng,
                                                        const int* __restrict__ dpos, unsigned seed0, unsigned seed1,
                                                        unsigned path0, double* uncond, double4* __restrict__ resid,
                                                        double* __restrict__ noise)
{
    const long k = (long)blockIdx.x * 64 + threadIdx.x;
    if (k >= kc) return;
    const double* pm = par + 3 * k;
    const double mu = pm[2];
    const RngKey key{seed0, seed1, path0 + (unsigned)k};
    double* f = uncond + k * (long)ng;
    simulate_car1(pm[0], pm[1], grid, ng, key, f);
    for (int j = 0; j < n; j++) {
        const double4 r = series[j];
        const double z = rng_normal(key, (uint64_t)j, 1);
        resid[k * (long)n + j] = make_double4(r.x, csim_resid(r.y, mu, f[dpos[j]], yerr[j], z), r.z, r.w);
        if (noise) noise[k * (long)n + j] = z;
    }
}

// One lane group per (path, time) pair e = k M + i: out[k][i] = f~_k(tsim_i) + E[f(tsim_i) | residual series k] + mu_k.
// spos[i] = position of tsim[i] in the merged grid.  The groups of a wave may belong to different paths; every residual
// series has n records, so the trip count of predict_run's loop is wave-uniform (its exchange needs that).
template <int P, int G>
__global__ __launch_bounds__(64) void k_csim_predict_carma(const double* __restrict__ par, int kc,
                                                           const double4* __restrict__ resid, int n,
                                                           const double* __restrict__ tsim, const int* __restrict__ spos, int M,
                                                           const double* __restrict__ uncond, int ng, double* __restrict__ out)
{
    __shared__ double4 xch[64];
    __shared__ double2 xch2[64];
    const int tid = threadIdx.x;
    Grp<G> g{xch, tid & 63, xch2};
    const long npairs = (long)kc * M;
    long e = ((long)blockIdx.x * 64 + tid) / G;
    const bool live = e < npairs;
    if (!live) e = npairs - 1;                                // (idle groups repeat the last pair and write nothing)
    const long k = e / M;
    const int i = (int)(e % M);
    const double* pm = par + k * (3 * P + 2);
    Model<P> m;
    model_from_roots<P, G>(g, pm, pm + 2 * P, pm[3 * P], m);
    double mean, var;
    bool sing;
    predict_run<P, G>(g, m, resid + k * (long)n, n, tsim[i], &mean, &var, &sing);
    if (live && g.lane() == 0) out[e] = add_back_mu(csim_add(uncond[k * (long)ng + spos[i]], mean), pm[3 * P + 1]);
}

__global__ __launch_bounds__(64) void k_csim_predict_car1(const double* __restrict__ par, int kc,
                                                          const double4* __restrict__ resid, int n,
                                                          const double* __restrict__ tsim, const int* __restrict__ spos, int M,
                                                          const double* __restrict__ uncond, int ng, double* __restrict__ out)
{
    const long e = (long)blockIdx.x * 64 + threadIdx.x;
    if (e >= (long)kc * M) return;
    const long k = e / M;
    const int i = (int)(e % M);
    const double* pm = par + 3 * k;
    double mean, var;
    predict_car1(pm[0], pm[1], resid + k * (long)n, n, tsim[i], &mean, &var);
    out[e] = add_back_mu(csim_add(uncond[k * (long)ng + spos[i]], mean), pm[2]);
}

// what the two launches of a chunk work on (device pointers)
struct CsimArgs {
    const double* par;        // rows of the chunk's first path on
    int kc;
    const double4* series;
    const double* yerr;
    int n;
    const double *grid, *tsim;
    const int *dpos, *spos;
    int ng, M;
    unsigned seed0, seed1, path0;
    double* uncond;
    double4* resid;
    double* noise;            // or null
    int* singular;            // the chunk's first flag on
    double* out;
};

template <int P>
static hipError_t launch_csim_p(const CsimArgs& a)
{
    constexpr int G = GroupOf<P>::value;
    const unsigned b1 = (unsigned)(((long)a.kc * G + 63) / 64);
    hipLaunchKernelGGL((k_csim_paths_carma<P, G>), dim3(b1), dim3(64), 0, nullptr, a.par, a.kc, a.series, a.yerr, a.n, a.grid,
                       a.ng, a.dpos, a.seed0, a.seed1, a.path0, a.uncond, a.resid, a.noise, a.singular);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned b2 = (unsigned)(((long)a.kc * a.M * G + 63) / 64);
    hipLaunchKernelGGL((k_csim_predict_carma<P, G>), dim3(b2), dim3(64), 0, nullptr, a.par, a.kc, a.resid, a.n, a.tsim, a.spos,
                       a.M, a.uncond, a.ng, a.out);
    return hipGetLastError();
}

static hipError_t launch_csim(int p, const CsimArgs& a)
{
    (void)hipGetLastError();   // HIP's last-error is sticky: drop anything left by earlier calls
    if (p == 1) {
        hipLaunchKernelGGL(k_csim_paths_car1, dim3((unsigned)(((long)a.kc + 63) / 64)), dim3(64), 0, nullptr, a.par, a.kc, a.series,
                           a.yerr, a.n, a.grid, a.ng, a.dpos, a.seed0, a.seed1, a.path0, a.uncond, a.resid, a.noise);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_csim_predict_car1, dim3((unsigned)(((long)a.kc * a.M + 63) / 64)), dim3(64), 0, nullptr, a.par, a.kc,
                           a.resid, a.n, a.tsim, a.spos, a.M, a.uncond, a.ng, a.out);
        return hipGetLastError();
    }
    return for_order(p, hipErrorInvalidValue, [&](auto P) { return launch_csim_p<decltype(P)::value>(a); });
}

// paths per chunk: the "CSIM_CHUNK_PATHS" switch, or as many as keep the scratch under the cap
static int csim_chunk_paths(size_t bytes_per_path, int npaths)
{
    const long t = tune_get(TUNE_CSIM_CHUNK_PATHS);
    long c = (t != TUNE_UNSET && t > 0) ? t : (long)std::max<size_t>(1, CSIM_SCRATCH_CAP / bytes_per_path);
    // (a launch's pair count kc M G / 64 workgroups must also fit the grid's 32 bits: far above any chunk under the cap)
    return (int)std::min<long>(c, npaths);
}

// par = [npaths][pw] rows as the kernels read them (validated, roots normalised); p == 1: pw = 3
static int csim_run(const char* who, const double* time, const double* y, const double* yerr, int n, int p, int npaths,
                    std::vector<double>& par, const double* tsim, int M, uint64_t seed, unsigned path0, double* out,
                    double* uncond, double* noise, int* singular, int* n_out, int device)
{
    for (int i = 0; i < M; i++) {
        if (!std::isfinite(tsim[i])) {
            set_error("%s: tsim[%d] is not finite", who, i);
            return CARMA_EINVAL;
        }
    }
    DevMem b_s, b_e, b_grid, b_tsim, b_pos, b_par, b_sing, b_unc, b_res, b_noise, b_out;
    std::vector<double> t(time, time + n), yy(y, y + n), ee(yerr, yerr + n);
    sort_dedup(t, yy, ee);
    const int m = (int)t.size();
    if (m < 2) {
        set_error("%s: fewer than 2 distinct data times", who);
        return CARMA_EINVAL;
    }
    if (n_out) *n_out = m;
    const int rc = select_device(device);
    if (rc != CARMA_OK) return rc;

    // merged grid: stable ascending sort of (data times, sorted tsim) -- a tsim equal to a datum comes behind it
    std::vector<int> perm(M);                                 // sorted tsim r = caller's tsim perm[r]
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return tsim[a] < tsim[b]; });
    const int ng = m + M;
    std::vector<double> cat(ng);
    for (int j = 0; j < m; j++) cat[j] = t[j];
    for (int r = 0; r < M; r++) cat[m + r] = tsim[perm[r]];
    std::vector<int> order(ng);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cat[a] < cat[b]; });
    std::vector<double> grid(ng);
    std::vector<int> pos(ng);                                 // [0, m): dpos; [m, ng): spos in the caller's order
    for (int i = 0; i < ng; i++) {
        grid[i] = cat[order[i]];
        const int src = order[i];
        pos[src < m ? src : m + perm[src - m]] = i;
    }
    const std::vector<double> s = pack_series(t, yy, ee);

    const int pw = (int)(par.size() / (size_t)npaths);
    const size_t per_path = (size_t)32 * m + (size_t)8 * ng + (noise ? (size_t)8 * m : 0);
    const int chunk = csim_chunk_paths(per_path, npaths);
    hipError_t e = b_s.alloc(sizeof(double) * s.size());
    if (e == hipSuccess) e = b_e.alloc(sizeof(double) * m);
    if (e == hipSuccess) e = b_grid.alloc(sizeof(double) * ng);
    if (e == hipSuccess) e = b_tsim.alloc(sizeof(double) * M);
    if (e == hipSuccess) e = b_pos.alloc(sizeof(int) * ng);
    if (e == hipSuccess) e = b_par.alloc(sizeof(double) * par.size());
    if (e == hipSuccess) e = b_sing.alloc(sizeof(int) * npaths);
    if (e == hipSuccess) e = b_unc.alloc(sizeof(double) * (size_t)chunk * ng);
    if (e == hipSuccess) e = b_res.alloc(sizeof(double) * 4 * (size_t)chunk * m);
    if (e == hipSuccess && noise) e = b_noise.alloc(sizeof(double) * (size_t)chunk * m);
    if (e == hipSuccess) e = b_out.alloc(sizeof(double) * (size_t)chunk * M);
    double *d_s = b_s.as<double>(), *d_e = b_e.as<double>(), *d_grid = b_grid.as<double>(), *d_tsim = b_tsim.as<double>(),
           *d_par = b_par.as<double>(), *d_unc = b_unc.as<double>(), *d_res = b_res.as<double>(), *d_noise = b_noise.as<double>(),
           *d_out = b_out.as<double>();
    int *d_pos = b_pos.as<int>(), *d_sing = b_sing.as<int>();
    if (e == hipSuccess) e = hipMemcpy(d_s, s.data(), sizeof(double) * s.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_e, ee.data(), sizeof(double) * m, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_grid, grid.data(), sizeof(double) * ng, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_tsim, tsim, sizeof(double) * M, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_pos, pos.data(), sizeof(int) * ng, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_sing, 0, sizeof(int) * npaths);
    for (int k0 = 0; k0 < npaths && e == hipSuccess; k0 += chunk) {
        const int kc = std::min(chunk, npaths - k0);
        CsimArgs a{};
        a.par = d_par + (size_t)k0 * pw;
        a.kc = kc;
        a.series = reinterpret_cast<const double4*>(d_s);
        a.yerr = d_e;
        a.n = m;
        a.grid = d_grid;
        a.tsim = d_tsim;
        a.dpos = d_pos;
        a.spos = d_pos + m;
        a.ng = ng;
        a.M = M;
        a.seed0 = (unsigned)(seed & 0xffffffffu);
        a.seed1 = (unsigned)(seed >> 32);
        a.path0 = path0 + (unsigned)k0;
        a.uncond = d_unc;
        a.resid = reinterpret_cast<double4*>(d_res);
        a.noise = d_noise;
        a.singular = d_sing + k0;
        a.out = d_out;
        e = launch_csim(p, a);
        if (e == hipSuccess) e = hipMemcpy(out + (size_t)k0 * M, d_out, sizeof(double) * (size_t)kc * M, hipMemcpyDeviceToHost);
        if (e == hipSuccess && uncond)
            e = hipMemcpy(uncond + (size_t)k0 * ng, d_unc, sizeof(double) * (size_t)kc * ng, hipMemcpyDeviceToHost);
        if (e == hipSuccess && noise)
            e = hipMemcpy(noise + (size_t)k0 * m, d_noise, sizeof(double) * (size_t)kc * m, hipMemcpyDeviceToHost);
    }
    std::vector<int> sing(npaths, 0);
    if (e == hipSuccess && p > 1) e = hipMemcpy(sing.data(), d_sing, sizeof(int) * npaths, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, who);
    bool any = false;
    for (int k = 0; k < npaths; k++) {
        any |= sing[k] != 0;
        if (singular) singular[k] = sing[k];
    }
    return (any && !singular) ? 1 : CARMA_OK;
}

}  // namespace carma

using namespace carma;

extern "C" {

int carma_simulate_cond_carma(const double* time, const double* y, const double* yerr, int n, int p, int npaths,
                              const double* sigsqr, const double* omega_re_im, const double* ma, int nma, const double* mu,
                              const double* tsim, int M, uint64_t seed, unsigned path0, double* out, double* uncond,
                              double* noise, int* singular, int* n_out, int device)
{
    static const char* const who = "carma_simulate_cond_carma";
    if (npaths < 1 || M < 1) {
        set_error("%s: need npaths >= 1 and M >= 1 (got npaths = %d, M = %d)", who, npaths, M);
        return CARMA_EINVAL;
    }
    if (!time || !y || !yerr || n < 2 || p < 2 || p > CARMA_PMAX || !sigsqr || !omega_re_im || !ma || !tsim || !out) {
        set_error("%s: bad argument (non-null arrays, n >= 2, 2 <= p <= %d)", who, CARMA_PMAX);
        return CARMA_EINVAL;
    }
    if (nma < 1 || nma > p) {
        set_error("%s: need 1 <= nma <= p (got nma = %d, p = %d)", who, nma, p);
        return CARMA_EINVAL;
    }
    const int pw = 3 * p + 2;
    std::vector<double> par((size_t)npaths * pw, 0.0);
    for (int k = 0; k < npaths; k++) {
        if (!(sigsqr[k] > 0.0)) {
            set_error("%s: path %d: need sigsqr > 0", who, k);
            return CARMA_EINVAL;
        }
        if (pack_model_row(p, omega_re_im + (size_t)k * 2 * p, ma + (size_t)k * nma, nma, sigsqr[k], mu ? mu[k] : 0.0,
                           par.data() + (size_t)k * pw) != CARMA_OK) {
            set_error("%s: path %d: the AR roots must be real or come in complex-conjugate pairs", who, k);
            return CARMA_EINVAL;
        }
    }
    return csim_run(who, time, y, yerr, n, p, npaths, par, tsim, M, seed, path0, out, uncond, noise, singular, n_out, device);
}

int carma_simulate_cond_car1(const double* time, const double* y, const double* yerr, int n, int npaths, const double* sigsqr,
                             const double* omega, const double* mu, const double* tsim, int M, uint64_t seed, unsigned path0,
                             double* out, double* uncond, double* noise, int* singular, int* n_out, int device)
{
    static const char* const who = "carma_simulate_cond_car1";
    if (npaths < 1 || M < 1) {
        set_error("%s: need npaths >= 1 and M >= 1 (got npaths = %d, M = %d)", who, npaths, M);
        return CARMA_EINVAL;
    }
    if (!time || !y || !yerr || n < 2 || !sigsqr || !omega || !tsim || !out) {
        set_error("%s: bad argument (non-null arrays, n >= 2)", who);
        return CARMA_EINVAL;
    }
    std::vector<double> par((size_t)npaths * 3, 0.0);
    for (int k = 0; k < npaths; k++) {
        if (!(sigsqr[k] > 0.0) || !(omega[k] > 0.0)) {
            set_error("%s: path %d: need sigsqr > 0 and omega > 0", who, k);
            return CARMA_EINVAL;
        }
        par[3 * (size_t)k] = sigsqr[k];
        par[3 * (size_t)k + 1] = omega[k];
        par[3 * (size_t)k + 2] = mu ? mu[k] : 0.0;
    }
    return csim_run(who, time, y, yerr, n, 1, npaths, par, tsim, M, seed, path0, out, uncond, noise, singular, n_out, device);
}

}  // extern "C"
