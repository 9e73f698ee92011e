// carma_mitems.hip -- Filter(), Predict and the one-pass smoother of MANY (series, model) items of a multi-series context
// (carma_mseries.hip) in one launch (carma_mkfilter, carma_mpredict, carma_msmooth).  The launch plans are
// host-only code in carma_mseries_plan.h; an entry point validates, plans, uploads / launches / downloads, and scatters the results.
//   - filter: one ITEM per lane -- kfilter_lane / car1_filter with a series pointer and a length of the lane's own.  The loop over
//     the data is a divergent one (a lane that has finished is masked off by the compiler's exec handling; nothing inside
//     lane_filter with in-line factors talks across lanes), the records come in with per-lane vector loads, and the host plan
//     sorts the items by length so that a wave's lanes finish together.  A wave writes into a tile of its own, [2 nmax_w][lanes]
//     (row k: mean_k of every lane; row n_l + k: var_k of lane l), so that the stores of a step are contiguous wherever the
//     lanes' lengths agree; k_mtranspose_mv then moves the tiles into the caller's ragged layout, 32 data of an item at a time;
//   - predict: one lane GROUP per (item, time) with predict_run; its group exchange needs one trip count per wave, so a wave
//     takes ONE series (wave table indexed by blockIdx.x) and its 64 / G groups take (item, time) pairs on that series;
//   - smooth: see k_msmooth_carma below.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "grp_device.h"
#include "carma_core.h"
#include "carma_lane.h"
#include "carma_predict.h"
#include "carma_smooth.h"
#include "carma_mseries.h"

namespace carma {

// Filter() of M items, one per lane.  par: per slot [M][3 P + 2] as k_kfilter_carma_lane takes it, slots in the plan's order (longest
// series first); slot_series[M]; tile_off[waves]: start of the wave's tile in mv.  Lanes past M leave after the barrier.
template <int P>
__global__ __launch_bounds__(64) void k_mkfilter_carma_lane(const double* __restrict__ par, int M, const double4* __restrict__ records,
                                                           const long* __restrict__ off, const int* __restrict__ nser,
                                                           const int* __restrict__ slot_series, const long* __restrict__ tile_off,
                                                           double* __restrict__ mv, int* __restrict__ singular)
{
    __shared__ double s_tab[MATH_TAB_N];
    math_tab_fill(s_tab);
    __syncthreads();
    const long slot = (long)blockIdx.x * 64 + threadIdx.x;
    if (slot >= M) return;
    const long ld = min(64L, (long)M - (long)blockIdx.x * 64);            // lanes of this wave that hold an item
    const int s = slot_series[slot];
    const double* pm = par + slot * (3 * P + 2);
    const bool sing = kfilter_lane<P>(pm, pm + 2 * P, pm[3 * P], pm[3 * P + 1], records + off[s], nser[s], s_tab,
                                      mv + tile_off[blockIdx.x] + threadIdx.x, ld);
    singular[slot] = sing ? 1 : 0;
}

// CAR(1): par = [M][3] (sigsqr, omega, mu), the same tiles
__global__ __launch_bounds__(64) void k_mkfilter_car1(const double* __restrict__ par, int M, const double4* __restrict__ records,
                                                      const long* __restrict__ off, const int* __restrict__ nser,
                                                      const int* __restrict__ slot_series, const long* __restrict__ tile_off,
                                                      double* __restrict__ mv)
{
    const long slot = (long)blockIdx.x * 64 + threadIdx.x;
    if (slot >= M) return;
    const long ld = min(64L, (long)M - (long)blockIdx.x * 64);
    const int s = slot_series[slot];
    const int n = nser[s];
    const double* pm = par + slot * 3;
    double* t = mv + tile_off[blockIdx.x] + threadIdx.x;
    (void)car1_filter(pm[0], pm[1], pm[2], 1.0, records + off[s], n, true, t, t + (long)n * ld, ld, true);
}

// The tiles of the filter kernels -> the caller's ragged arrays: the item in lane l of wave blockIdx.x has slot_n data, its
// means go to mean[slot_out + k], its variances to var[slot_out + k].  32 rows of a tile at a time through LDS: the reads
// follow the tile's rows, the writes put 32 consecutive data of one item side by side; nothing is written at or past k = n_l.
__global__ __launch_bounds__(256) void k_mtranspose_mv(const double* __restrict__ mv, const long* __restrict__ tile_off, int M,
                                                       const int* __restrict__ slot_n, const long* __restrict__ slot_out,
                                                       double* __restrict__ mean, double* __restrict__ var)
{
    __shared__ double s_m[32][65], s_v[32][65];
    __shared__ int s_n[64];
    __shared__ long s_o[64];
    const long slot0 = (long)blockIdx.x * 64;
    const int ld = (int)min(64L, (long)M - slot0);
    if (threadIdx.x < 64) {
        const bool live = (int)threadIdx.x < ld;
        s_n[threadIdx.x] = live ? slot_n[slot0 + threadIdx.x] : 0;
        s_o[threadIdx.x] = live ? slot_out[slot0 + threadIdx.x] : 0;
    }
    __syncthreads();
    const int nmax = s_n[0];                                  // the plan sorts by length: lane 0 holds the wave's longest
    const double* tile = mv + tile_off[blockIdx.x];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;   // reading: 64 lanes x 4 rows
    const int kx = threadIdx.x & 31, ly = threadIdx.x >> 5;   // writing: 32 data x 8 items
    for (int k0 = blockIdx.y * 32; k0 < nmax; k0 += gridDim.y * 32) {
        const int ntx = s_n[tx];
        for (int j = ty; j < 32; j += 4) {
            const int k = k0 + j;
            if (k < ntx) {
                s_m[j][tx] = tile[(long)k * ld + tx];
                s_v[j][tx] = tile[((long)ntx + k) * ld + tx];
            }
        }
        __syncthreads();
        const int k = k0 + kx;
        for (int l = ly; l < ld; l += 8) {
            if (k < s_n[l]) {
                mean[s_o[l] + k] = s_m[kx][l];
                var[s_o[l] + k] = s_v[kx][l];
            }
        }
        __syncthreads();
    }
}

// Predict of (item, time) pairs: wave blockIdx.x works on series wave_series[blockIdx.x], its 64 / G groups on the pairs
// pair_out[64 / G * blockIdx.x + group] (index into tpred / pmean / pvar; -1: an idle group, which repeats the wave's first
// pair and writes nothing) of item pair_item[.].  par = [items][3 P + 2] in the caller's order.
template <int P, int G>
__global__ __launch_bounds__(64) void k_mpredict_carma(const double* __restrict__ par, const double4* __restrict__ records,
                                                      const long* __restrict__ off, const int* __restrict__ nser,
                                                      const int* __restrict__ wave_series, const int* __restrict__ pair_item,
                                                      const long* __restrict__ pair_out, const double* __restrict__ tpred,
                                                      double* __restrict__ pmean, double* __restrict__ pvar, int* __restrict__ singular)
{
    __shared__ double4 xch[64];
    __shared__ double2 xch2[64];
    const int tid = threadIdx.x;
    Grp<G> g{xch, tid & 63, xch2};
    const int s = wave_series[blockIdx.x];                    // wave-uniform: one trip count for every group (predict_run's exchange)
    const double4* series = records + off[s];
    const int n = nser[s];
    long e = (long)blockIdx.x * (64 / G) + tid / G;
    const bool live = pair_out[e] >= 0;
    if (!live) e = (long)blockIdx.x * (64 / G);               // (group 0 of a wave is always live)
    const int item = pair_item[e];
    const long o = pair_out[e];
    const double* pm = par + (long)item * (3 * P + 2);
    Model<P> m;
    model_from_roots<P, G>(g, pm, pm + 2 * P, pm[3 * P], m);
    double mean, var;
    bool sing;
    predict_run<P, G>(g, m, series, n, tpred[o], &mean, &var, &sing, pm[3 * P + 1]);
    if (live && g.lane() == 0) {
        pmean[o] = mean;
        pvar[o] = var;
        if (sing) singular[item] = 1;
    }
}

// CAR(1): one lane per (item, time) pair, pairs in the caller's order; par = [items][3] (sigsqr, omega, mu)
__global__ __launch_bounds__(64) void k_mpredict_car1(const double* __restrict__ par, const double4* __restrict__ records,
                                                      const long* __restrict__ off, const int* __restrict__ nser,
                                                      const int* __restrict__ item_series, const int* __restrict__ pair_item,
                                                      long npairs, const double* __restrict__ tpred, double* __restrict__ pmean,
                                                      double* __restrict__ pvar)
{
    const long e = (long)blockIdx.x * 64 + threadIdx.x;
    if (e >= npairs) return;
    const int item = pair_item[e];
    const int s = item_series[item];
    const double* pm = par + 3L * item;
    predict_car1(pm[0], pm[1], records + off[s], nser[s], tpred[e], pmean + e, pvar + e, pm[2]);
}

// ---- the one-pass smoother over many (series, model) items (carma_msmooth) -----------------------------------------------
// A JOB is a (series, list of requested times) pair with its merged grid (carma_smooth_plan.h); the items that share a job fill
// waves of E = 64 / G groups (CAR(1): 64 lanes), so that a wave's loop over the grid is uniform; other items get waves of their
// own.  Wave w0 + blockIdx.x of the plan: job wave_job[w]; slot e of it: item slot_item[w E + e] (-1: idle, repeats the wave's
// first item and stores no output), outputs at slot_out[w E + e]; its scratch starts wave_pts[w] grid points into the chunk's.
// The device functions and the series records are those of carma_smooth_*: an item gets the bits of that call on its series.
struct MsmoothTabs {
    const int *wave_job, *job_series, *job_ng, *slot_item, *src;
    const long *job_goff, *slot_out, *wave_pts;
    const double* grid;
};

template <int P, int G>
__global__ __launch_bounds__(64) void k_msmooth_carma(const double* __restrict__ par, const double4* __restrict__ records,
                                                      const long* __restrict__ off, MsmoothTabs tb, long w0,
                                                      double4* __restrict__ rec, double4* __restrict__ grp,
                                                      double* __restrict__ mean, double* __restrict__ var,
                                                      int* __restrict__ singular)
{
    __shared__ double4 xch[64];
    __shared__ double2 xch2[64];
    constexpr int E = 64 / G;
    const int tid = threadIdx.x;
    Grp<G> g{xch, tid & 63, xch2};
    const long w = w0 + blockIdx.x;
    const int j = tb.wave_job[w];
    const double4* series = records + off[tb.job_series[j]];
    const int ng = tb.job_ng[j];
    const double* grid = tb.grid + tb.job_goff[j];
    const int* src = tb.src + tb.job_goff[j];
    const int e = tid / G;
    int item = tb.slot_item[w * E + e];
    const bool live = item >= 0;
    if (!live) item = tb.slot_item[w * E];                    // (slot 0 of a wave is always live)
    const double* pm = par + (long)item * (3 * P + 2);
    Model<P> m;
    model_from_roots<P, G>(g, pm, pm + 2 * P, pm[3 * P], m);
    const double mu = pm[3 * P + 1];
    FilterConsts<P> fc;
    filter_reset<P, G>(g, m, fc);
    double4* myrec = rec + (size_t)tb.wave_pts[w] * 64 + tid;
    double4* mygrp = grp + (size_t)tb.wave_pts[w] * E + e;
    smooth_forward<P, G>(g, m, fc, series, grid, src, ng, mu, myrec, 64, mygrp, E);
    __syncthreads();                                          // lane 0 wrote the group records, every lane of the group reads them
    const long o = tb.slot_out[w * E + e];
    smooth_backward<P, G>(g, fc, src, ng, mu, myrec, 64, mygrp, E, live ? mean + o : nullptr, live ? var + o : nullptr);
    if (live && g.lane() == 0) singular[item] = fc.sing ? 1 : 0;
}

// CAR(1): one lane per item; the wave's scratch is five planes of ng x 64 doubles
__global__ __launch_bounds__(64) void k_msmooth_car1(const double* __restrict__ par, const double4* __restrict__ records,
                                                     const long* __restrict__ off, MsmoothTabs tb, long w0, double* __restrict__ sc,
                                                     double* __restrict__ mean, double* __restrict__ var)
{
    const long w = w0 + blockIdx.x;
    const int j = tb.wave_job[w];
    const double4* series = records + off[tb.job_series[j]];
    const int ng = tb.job_ng[j];
    int item = tb.slot_item[w * 64 + threadIdx.x];
    const bool live = item >= 0;
    if (!live) item = tb.slot_item[w * 64];
    const double* pm = par + 3L * item;
    const long o = tb.slot_out[w * 64 + threadIdx.x];
    smooth_car1(pm[0], pm[1], pm[2], series, tb.grid + tb.job_goff[j], tb.src + tb.job_goff[j], ng,
                sc + (size_t)tb.wave_pts[w] * 64 * 5 + threadIdx.x, 64, 64L * ng, live ? mean + o : nullptr, live ? var + o : nullptr);
}

}  // namespace carma

using namespace carma;

extern "C" {

int carma_mkfilter(carma_mctx* h, const int* series, int M, const double* sigsqr, const double* omega_re_im, const double* ma,
                   int nma, const double* mu, double* mean, double* var, long* out_offsets, int* singular)
{
    static const char* const who = "carma_mkfilter";
    if (!h || !mean || !var) {
        set_error("%s: bad argument (null context or output)", who);
        return CARMA_EINVAL;
    }
    Mctx* c = reinterpret_cast<Mctx*>(h);
    const int p = c->p, PW = p == 1 ? 3 : 3 * p + 2;
    std::vector<double> par;
    int rc = pack_items(c, who, series, M, sigsqr, omega_re_im, ma, nma, mu, par);
    if (rc != CARMA_OK) return rc;
    const MfilterPlan pl = mfilter_plan(series, M, c->n.data());
    const long W = pl.W, total = pl.offs[M];
    std::vector<double> spar((size_t)M * PW);                 // the parameters in slot order
    for (long j = 0; j < M; j++) std::memcpy(&spar[(size_t)j * PW], &par[(size_t)pl.order[j] * PW], sizeof(double) * PW);
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    hipStream_t st = c->stream;
    std::vector<int> sing((size_t)M, 0);
    e = upload(c->k_par, spar, st);
    if (e == hipSuccess) e = upload(c->k_int, pl.tint, st);
    if (e == hipSuccess) e = upload(c->k_long, pl.tlong, st);
    if (e == hipSuccess) e = c->k_tile.need(sizeof(double) * pl.tile_total);
    if (e == hipSuccess) e = c->k_res.need(sizeof(double) * 2 * (size_t)total);
    if (e == hipSuccess) e = c->k_sing.need(sizeof(int) * (size_t)M);
    if (e == hipSuccess) {
        (void)hipGetLastError();   // HIP's last-error is sticky: drop anything left by earlier calls
        const double* d_par = c->k_par.as<double>();
        const int *d_sser = c->k_int.as<int>(), *d_sn = d_sser + M;
        const long *d_toff = c->k_long.as<long>(), *d_sout = d_toff + W;
        double *d_mv = c->k_tile.as<double>(), *d_mean = c->k_res.as<double>(), *d_var = d_mean + total;
        const dim3 grid((unsigned)W), block(64);
        if (p == 1) {
            hipLaunchKernelGGL(k_mkfilter_car1, grid, block, 0, st, d_par, M, c->rec(), c->offs(), c->ns(), d_sser, d_toff, d_mv);
            e = hipGetLastError();
        } else {
            e = for_order(p, hipErrorInvalidValue, [&](auto P) {
                hipLaunchKernelGGL((k_mkfilter_carma_lane<decltype(P)::value>), grid, block, 0, st, d_par, M, c->rec(), c->offs(), c->ns(),
                                   d_sser, d_toff, d_mv, c->k_sing.as<int>());
                return hipGetLastError();
            });
        }
        if (e == hipSuccess) {
            const dim3 tgrid((unsigned)W, (unsigned)std::min((pl.nmax + 31) / 32, 1024L));
            hipLaunchKernelGGL(k_mtranspose_mv, tgrid, dim3(256), 0, st, d_mv, d_toff, M, d_sn, d_sout, d_mean, d_var);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(mean, d_mean, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(var, d_var, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && p > 1)
            e = hipMemcpyAsync(sing.data(), c->k_sing.as<int>(), sizeof(int) * (size_t)M, hipMemcpyDeviceToHost, st);
    }
    rc = finish_items(who, e, st);
    if (rc != CARMA_OK) return rc;
    if (out_offsets) std::memcpy(out_offsets, pl.offs.data(), sizeof(long) * ((size_t)M + 1));
    if (singular)
        for (long j = 0; j < M; j++) singular[pl.order[j]] = sing[j];
    return CARMA_OK;
}

int carma_mpredict(carma_mctx* h, const int* series, int M, const double* sigsqr, const double* omega_re_im, const double* ma,
                   int nma, const double* mu, const double* tpred, const long* toff, double* pmean, double* pvar, int* singular)
{
    static const char* const who = "carma_mpredict";
    if (!h || !toff) {
        set_error("%s: bad argument (null context or toff)", who);
        return CARMA_EINVAL;
    }
    Mctx* c = reinterpret_cast<Mctx*>(h);
    const int p = c->p;
    std::vector<double> par;
    int rc = pack_items(c, who, series, M, sigsqr, omega_re_im, ma, nma, mu, par);
    if (rc == CARMA_OK) rc = toff_ok(who, toff, M);
    if (rc != CARMA_OK) return rc;
    const long t0 = toff[0], T = toff[M] - t0;
    if (T > 0 && (!tpred || !pmean || !pvar)) {
        set_error("%s: bad argument (null tpred, pmean or pvar)", who);
        return CARMA_EINVAL;
    }
    if (singular) std::fill(singular, singular + M, 0);
    if (T == 0) return CARMA_OK;
    const MpredictPlan pl = mpredict_plan(p == 1 ? 0 : group_of(p), series, M, c->S, c->n.data(), toff, c->wb.plan.b);
    const long W = pl.W;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    hipStream_t st = c->stream;
    std::vector<int> sing((size_t)M, 0);
    const size_t npar = par.size();
    e = c->k_par.need(sizeof(double) * (npar + (size_t)T));
    if (e == hipSuccess) e = hipMemcpyAsync(c->k_par.as<void>(), par.data(), sizeof(double) * npar, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->k_par.as<double>() + npar, tpred + t0, sizeof(double) * (size_t)T, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = upload(c->k_int, pl.tint, st);
    if (e == hipSuccess && p > 1) e = upload(c->k_long, pl.tlong, st);
    if (e == hipSuccess) e = c->k_res.need(sizeof(double) * 2 * (size_t)T);
    if (e == hipSuccess) e = c->k_sing.need(sizeof(int) * (size_t)M);
    if (e == hipSuccess) e = hipMemsetAsync(c->k_sing.as<int>(), 0, sizeof(int) * (size_t)M, st);
    if (e == hipSuccess) {
        (void)hipGetLastError();
        const double *d_par = c->k_par.as<double>(), *d_tp = d_par + npar;
        double *d_pm = c->k_res.as<double>(), *d_pv = d_pm + T;
        const int* d_int = c->k_int.as<int>();
        const dim3 grid((unsigned)W), block(64);
        if (p == 1) {
            hipLaunchKernelGGL(k_mpredict_car1, grid, block, 0, st, d_par, c->rec(), c->offs(), c->ns(), d_int, d_int + M, T, d_tp, d_pm,
                               d_pv);
            e = hipGetLastError();
        } else {
            e = for_order(p, hipErrorInvalidValue, [&](auto P) {
                constexpr int N = decltype(P)::value;
                hipLaunchKernelGGL((k_mpredict_carma<N, GroupOf<N>::value>), grid, block, 0, st, d_par, c->rec(), c->offs(), c->ns(), d_int,
                                   d_int + W, c->k_long.as<long>(), d_tp, d_pm, d_pv, c->k_sing.as<int>());
                return hipGetLastError();
            });
        }
        if (e == hipSuccess) e = hipMemcpyAsync(pmean + t0, d_pm, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(pvar + t0, d_pv, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(sing.data(), c->k_sing.as<int>(), sizeof(int) * (size_t)M, hipMemcpyDeviceToHost, st);
    }
    rc = finish_items(who, e, st);
    if (rc == CARMA_OK && singular) std::memcpy(singular, sing.data(), sizeof(int) * (size_t)M);
    return rc;
}

int carma_msmooth(carma_mctx* h, const int* series, int M, const double* sigsqr, const double* omega_re_im, const double* ma,
                  int nma, const double* mu, const double* tout, const long* toff, double* mean, double* var, int* singular)
{
    static const char* const who = "carma_msmooth";
    if (!h || !toff) {
        set_error("%s: bad argument (null context or toff)", who);
        return CARMA_EINVAL;
    }
    Mctx* c = reinterpret_cast<Mctx*>(h);
    const int p = c->p;
    std::vector<double> par;
    int rc = pack_items(c, who, series, M, sigsqr, omega_re_im, ma, nma, mu, par);
    if (rc == CARMA_OK) rc = toff_ok(who, toff, M);
    if (rc != CARMA_OK) return rc;
    const long t0 = toff[0], T = toff[M] - t0;
    if (T > 0 && (!tout || !mean || !var)) {
        set_error("%s: bad argument (null tout, mean or var)", who);
        return CARMA_EINVAL;
    }
    for (int i = 0; i < M; i++)
        for (long o = toff[i]; o < toff[i + 1]; o++)
            if (!std::isfinite(tout[o])) {
                set_error("%s: item %d: tout[%ld] is not finite", who, i, o);
                return CARMA_EINVAL;
            }
    if (singular) std::fill(singular, singular + M, 0);
    if (T == 0) return CARMA_OK;
    // (the "SMOOTH_CHUNK_MODELS" switch, or TUNE_UNSET < 0: chunks as large as the scratch cap allows)
    const int G = p > 1 ? group_of(p) : 0;
    const MsmoothPlan pl = msmooth_plan(G, series, M, tout, toff, c->t.data(), c->hoff.data(), c->n.data(), tune_get(TUNE_SMOOTH_CHUNK_MODELS));
    const long W = pl.W, J = pl.J, E = pl.E;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    hipStream_t st = c->stream;
    std::vector<int> sing((size_t)M, 0);
    const size_t npar = par.size();
    e = c->k_par.need(sizeof(double) * (npar + pl.grids.size()));
    if (e == hipSuccess) e = hipMemcpyAsync(c->k_par.as<void>(), par.data(), sizeof(double) * npar, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->k_par.as<double>() + npar, pl.grids.data(), sizeof(double) * pl.grids.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = upload(c->k_int, pl.tint, st);
    if (e == hipSuccess) e = upload(c->k_long, pl.tlong, st);
    if (e == hipSuccess) e = c->k_tile.need(smooth_wave_bytes(G, 1) * pl.pts_max);
    if (e == hipSuccess) e = c->k_res.need(sizeof(double) * 2 * (size_t)T);
    if (e == hipSuccess) e = c->k_sing.need(sizeof(int) * (size_t)M);
    if (e == hipSuccess) e = hipMemsetAsync(c->k_sing.as<int>(), 0, sizeof(int) * (size_t)M, st);
    if (e == hipSuccess) {
        (void)hipGetLastError();
        const double* d_par = c->k_par.as<double>();
        const int* di = c->k_int.as<int>();
        const long* dl = c->k_long.as<long>();
        MsmoothTabs tb;
        tb.wave_job = di;
        tb.job_series = di + W;
        tb.job_ng = tb.job_series + J;
        tb.slot_item = tb.job_ng + J;
        tb.src = tb.slot_item + W * E;
        tb.job_goff = dl;
        tb.slot_out = dl + J;
        tb.wave_pts = tb.slot_out + W * E;
        tb.grid = d_par + npar;
        double *d_m = c->k_res.as<double>(), *d_v = d_m + T;
        // a chunk's scratch: the lane records of its waves, then their group records
        double4* rec = c->k_tile.as<double4>();
        double4* grp = rec + pl.pts_max * 64;
        for (size_t ci = 0; ci + 1 < pl.chunk0.size() && e == hipSuccess; ci++) {
            const long w0 = pl.chunk0[ci];
            const dim3 grid((unsigned)(pl.chunk0[ci + 1] - w0)), block(64);
            if (p == 1) {
                hipLaunchKernelGGL(k_msmooth_car1, grid, block, 0, st, d_par, c->rec(), c->offs(), tb, w0, c->k_tile.as<double>(), d_m,
                                   d_v);
                e = hipGetLastError();
            } else {
                e = for_order(p, hipErrorInvalidValue, [&](auto P) {
                    constexpr int N = decltype(P)::value;
                    hipLaunchKernelGGL((k_msmooth_carma<N, GroupOf<N>::value>), grid, block, 0, st, d_par, c->rec(), c->offs(), tb, w0, rec,
                                       grp, d_m, d_v, c->k_sing.as<int>());
                    return hipGetLastError();
                });
            }
        }
        if (e == hipSuccess) e = hipMemcpyAsync(mean + t0, d_m, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(var + t0, d_v, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(sing.data(), c->k_sing.as<int>(), sizeof(int) * (size_t)M, hipMemcpyDeviceToHost, st);
    }
    rc = finish_items(who, e, st);
    if (rc == CARMA_OK && singular) std::memcpy(singular, sing.data(), sizeof(int) * (size_t)M);
    return rc;
}

}  // extern "C"
