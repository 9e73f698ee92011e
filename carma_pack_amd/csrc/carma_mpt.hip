// carma_mpt.hip -- the SAMPLER over many series (carma_mpt_*) of a multi-series context
// (carma_mseries.hip): the large-ensemble sampler of carma_pt_lane.hip -- one chain per
// lane, an iteration as k_ram_propose / K1 / k_ram_finish -- with a K1 in which every chain is evaluated on the series of its own
// ladder (k_logdens_carma_chains_ms).  A RUN is one sampler (R replicas x T temperatures) on one series; a call's M runs are the
// ladders j R .. j R + R - 1 of ONE ensemble of M R ladders, so the bookkeeping kernels, the Philox keys and the start-value keys
// are those of a single-series ensemble of that size, and run j is its block replica0 = j R.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "grp_device.h"
#include "carma_core.h"
#include "carma_lane.h"
#include "carma_mseries.h"

namespace carma {

// K1 of the multi-series sampler: ONE CHAIN PER LANE, chain gi = 64 blockIdx.x + threadIdx.x of the ensemble, on the series of its
// ladder, ladder_series[gi / T].  thn = [nc][d] chain-major (the proposals k_ram_propose / k_ram_finish write), ll = [nc].
//   - the series' offset, length and prior are per-lane values and the records come in with per-lane vector loads (the lanes of a
//     ladder share an address); the loop over the data is a divergent one that ends at the wave's longest series;
//   - logdensity_lane has ONE wave-wide operation, the ballot "does any lane have a real pair" in front of the loop, and what it
//     guards only ever changes lanes that have such a pair: its outcome cannot change a lane's bits, whatever the lanes' lengths;
//   - REPDT is a property of the SERIES (rep[s], as carma_ctx_create decides it) and selects another instruction stream, so the
//     regular-cadence series' chains are served by a launch of their own: a lane whose series belongs to the other launch leaves
//     (after the barrier), a wave without any lane of this launch is gone at once.  A chain gets the bits of the single-series lane
//     kernel on its series, as k_logdens_carma_lane_ms gives them;
//   - lanes past nc shadow the last chain and write nothing.
template <int P, bool REPDT>
__global__ __launch_bounds__(64) void k_logdens_carma_chains_ms(const double* __restrict__ thn, int d, int q, long nc, int T,
                                                               const double4* __restrict__ records, const long* __restrict__ off,
                                                               const int* __restrict__ nser, const Prior* __restrict__ prs,
                                                               const char* __restrict__ rep, const int* __restrict__ ladder_series,
                                                               double* __restrict__ ll)
{
    __shared__ double s_tab[MATH_TAB_N];                     // tables of the table-based exp / sincos (carma_math.h)
    math_tab_fill(s_tab);
    __syncthreads();
    long gi = (long)blockIdx.x * 64 + threadIdx.x;
    const bool live = gi < nc;
    if (!live) gi = nc - 1;
    const int s = ladder_series[gi / T];
    if ((rep[s] != 0) != REPDT) return;
    const double v = logdensity_lane<P, REPDT>(thn + gi * d, q, records + off[s], nser[s], prs[s], 0, s_tab);
    if (live) ll[gi] = v;
}

__global__ __launch_bounds__(64) void k_logdens_car1_chains_ms(const double* __restrict__ thn, long nc, int T,
                                                              const double4* __restrict__ records, const long* __restrict__ off,
                                                              const int* __restrict__ nser, const Prior* __restrict__ prs,
                                                              const int* __restrict__ ladder_series, double* __restrict__ ll)
{
    long gi = (long)blockIdx.x * 64 + threadIdx.x;
    const bool live = gi < nc;
    if (!live) gi = nc - 1;
    const int s = ladder_series[gi / T];
    const double v = logdensity_car1(thn + 4 * gi, records + off[s], nser[s], prs[s]);
    if (live) ll[gi] = v;
}

// ---- the sampler over many series -------------------------------------------------------------------------------------
// K1: every chain of the ensemble on its ladder's series; the regular-cadence series' chains in a launch of their own
static hipError_t launch_logdens_chains_ms(const Mctx* c, const MptState* s, const double* thn, long nc, double* ll, hipStream_t st)
{
    (void)hipGetLastError();   // HIP's last-error is sticky: drop anything left by earlier calls
    const dim3 grid((unsigned)((nc + 63) / 64)), block(64);
    if (c->p == 1) {
        hipLaunchKernelGGL(k_logdens_car1_chains_ms, grid, block, 0, st, thn, nc, s->T, c->rec(), c->offs(), c->ns(), c->prs(),
                           s->d_lser.get(), ll);
        return hipGetLastError();
    }
    for (int rep = 0; rep < 2; rep++) {
        if (!(rep ? s->any_rep : s->any_plain)) continue;
        const hipError_t e = for_order(c->p, hipErrorInvalidValue, [&](auto P) {
            if (rep)
                hipLaunchKernelGGL((k_logdens_carma_chains_ms<decltype(P)::value, true>), grid, block, 0, st, thn, c->d, c->q, nc, s->T,
                                   c->rec(), c->offs(), c->ns(), c->prs(), s->d_rep.get(), s->d_lser.get(), ll);
            else
                hipLaunchKernelGGL((k_logdens_carma_chains_ms<decltype(P)::value, false>), grid, block, 0, st, thn, c->d, c->q, nc, s->T,
                                   c->rec(), c->offs(), c->ns(), c->prs(), s->d_rep.get(), s->d_lser.get(), ll);
            return hipGetLastError();
        });
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// the sampler state of h, or null with the error set: `who` was called before carma_mpt_create (need_start: or before the
// chains have starting values)
static MptState* mpt_state(carma_mctx* h, const char* who, bool need_start)
{
    if (!h) {
        set_error("%s: null context", who);
        return nullptr;
    }
    MptState* s = reinterpret_cast<Mctx*>(h)->mpt.get();
    if (!s) {
        set_error("%s: call carma_mpt_create first", who);
        return nullptr;
    }
    if (need_start && !s->started) {
        set_error("%s: chains have no starting values (carma_mpt_start / carma_mpt_set_chains)", who);
        return nullptr;
    }
    return s;
}

// Iterations per chunk: the K1 of an iteration runs as long as its longest series (>= ~0.45 us per datum, as chunk_iters of the
// single-series lane sampler), 2-3 launches each; around a quarter of a second, at most 4096 iterations, are in flight at a time.
static long mpt_chunk_iters(const MptState* s)
{
    const double est_us = std::max(1.0, 0.45 * s->nmax);
    return (long)std::max(1.0, std::min(4096.0, 250000.0 / est_us));
}

// niter iterations, a chunk in flight at a time.  thin > 0: save the coldest chains every thin iterations from sample *save_offset on
static int mpt_iterate(Mctx* c, long niter, int do_exchange, int thin, long* save_offset)
{
    MptState* s = c->mpt.get();
    const long chunk0 = mpt_chunk_iters(s);
    const PtLaneK1 k1 = [c, s](const double* thn, long nc, double* ll, hipStream_t st) {
        return launch_logdens_chains_ms(c, s, thn, nc, ll, st);
    };
    long left = niter;
    while (left > 0) {
        const long ch = pt_next_chunk(left, chunk0, thin);
        const PtLaunch L = pt_ens_launch(s, c->d, c->q, s->nmax, ch, do_exchange, thin, save_offset ? *save_offset : 0);
        hipError_t e = launch_pt_lane_k1(c->p, L, s->d_scratch, k1, pt_ens_buffers(s), !s->factor_loaded, c->stream);
        if (e == hipSuccess) {
            s->factor_loaded = true;
            s->chol_stale = true;
            e = hipStreamSynchronize(c->stream);
        }
        if (e != hipSuccess) return hip_fail(e, "carma_mpt: sampler launch");
        pt_ens_advance(s, ch, thin, save_offset);
        left -= ch;
    }
    return CARMA_OK;
}

}  // namespace carma

using namespace carma;

extern "C" {

int carma_mpt_create(carma_mctx* h, const int* series, int M, int ntemps, int nreplicas, const double* temperatures, int adapt_iters,
                     uint64_t seed)
{
    if (!h || !series || nreplicas < 1 || adapt_iters < 0) {
        set_error("carma_mpt_create: bad argument (null context or series, nreplicas < 1 or adapt_iters < 0)");
        return CARMA_EINVAL;
    }
    if (M < 1) {
        set_error("carma_mpt_create: need at least one run (got M = %d)", M);
        return CARMA_EINVAL;
    }
    if (ntemps < 1 || ntemps > 64) {
        set_error("carma_mpt_create: a ladder is 1 ... 64 temperatures, the lanes of a wave (got %d)", ntemps);
        return CARMA_EINVAL;
    }
    Mctx* c = reinterpret_cast<Mctx*>(h);
    for (int j = 0; j < M; j++)
        if (series[j] < 0 || series[j] >= c->S) {
            set_error("carma_mpt_create: run %d: series index %d out of range (nseries = %d)", j, series[j], c->S);
            return CARMA_EINVAL;
        }
    // (chain and ladder indices are ints in the launch arguments, evaluation counts in carma_mlogdensity_batch too)
    const long long nc_ll = (long long)M * nreplicas * ntemps;
    if (nc_ll > 0x7fffffffLL - 64) {
        set_error("carma_mpt_create: %d runs x %d replicas x %d temperatures = %lld chains, more than one launch can index (%lld)", M,
                  nreplicas, ntemps, nc_ll, 0x7fffffffLL - 64);
        return CARMA_EINVAL;
    }
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    c->mpt.reset(new MptState());         // (the state of an earlier call goes, with every buffer it holds)
    MptState* s = c->mpt.get();
    s->M = M;
    s->reps = nreplicas;
    s->maxiter = adapt_iters;
    s->seed = seed;
    s->series.assign(series, series + M);
    std::vector<double> temps;
    default_ladder(ntemps, temperatures, temps);             // shared by all runs
    const int d = c->d, nlad = M * nreplicas;
    const size_t nchain = (size_t)nc_ll;
    // initial proposal factor of run j, from ITS series
    std::vector<double> chol(nchain * d * d, 0.0), R0((size_t)d * d);
    std::vector<int> lser((size_t)nlad);
    for (int j = 0; j < M; j++) {
        const int sj = series[j];
        const long n = c->n[sj];
        s->nmax = std::max(s->nmax, (int)n);
        (c->repdt[sj] ? s->any_rep : s->any_plain) = true;
        initial_factor(pop_var(c->y.data() + c->hoff[sj], n), n, d, R0.data());
        for (size_t k = (size_t)j * nreplicas * ntemps; k < (size_t)(j + 1) * nreplicas * ntemps; k++)
            std::memcpy(&chol[k * d * d], R0.data(), sizeof(double) * d * d);
        for (int r = 0; r < nreplicas; r++) lser[(size_t)j * nreplicas + r] = sj;
    }
    e = pt_ens_create(s, ntemps, nlad, d, temps, chol.data());
    if (e == hipSuccess) e = s->d_lser.alloc(lser.size());
    if (e == hipSuccess) e = s->d_rep.alloc((size_t)c->S);
    if (e == hipSuccess) e = s->d_scratch.alloc(pt_lane_scratch_doubles(d, (long)nchain));
    if (e == hipSuccess) e = hipMemcpy(s->d_lser, lser.data(), sizeof(int) * lser.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_rep, c->repdt.data(), sizeof(char) * (size_t)c->S, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        c->mpt.reset();
        return hip_fail(e, "carma_mpt_create");
    }
    return CARMA_OK;
}

int carma_mpt_set_chains(carma_mctx* h, const double* theta, const double* logpost)
{
    MptState* s = mpt_state(h, "carma_mpt_set_chains", false);
    if (!s) return CARMA_EINVAL;
    if (!theta) {
        set_error("carma_mpt_set_chains: null theta");
        return CARMA_EINVAL;
    }
    Mctx* c = reinterpret_cast<Mctx*>(h);
    const size_t nchain = s->nchain();
    std::vector<double> lp(nchain);
    if (logpost) {
        std::memcpy(lp.data(), logpost, sizeof(double) * nchain);
    } else {
        std::vector<int> which(nchain);
        for (size_t k = 0; k < nchain; k++) which[k] = s->series[k / ((size_t)s->reps * s->T)];
        const int rc = carma_mlogdensity_batch(h, theta, which.data(), (int)nchain, 0, lp.data());
        if (rc != CARMA_OK) return rc;
    }
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = pt_ens_set_chains(s, c->d, theta, lp.data());
    if (e != hipSuccess) return hip_fail(e, "carma_mpt_set_chains");
    s->started = true;
    return CARMA_OK;
}

int carma_mpt_get_chains(carma_mctx* h, double* theta, double* logpost)
{
    MptState* s = mpt_state(h, "carma_mpt_get_chains", false);
    if (!s) return CARMA_EINVAL;
    Mctx* c = reinterpret_cast<Mctx*>(h);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = pt_ens_get_chains(s, c->d, theta, logpost);
    if (e != hipSuccess) return hip_fail(e, "carma_mpt_get_chains");
    return CARMA_OK;
}

int carma_mpt_start(carma_mctx* h, const double* init)
{
    MptState* s = mpt_state(h, "carma_mpt_start", false);
    if (!s) return CARMA_EINVAL;
    Mctx* c = reinterpret_cast<Mctx*>(h);
    const int d = c->d, M = s->M;
    const size_t per_run = (size_t)s->reps * s->T, nchain = s->nchain();
    std::vector<double> theta(nchain * d), lp(nchain, -std::numeric_limits<double>::infinity());
    std::vector<char> done(nchain, 0);
    // a run's init row is honoured when its log-density on the run's series is finite (src/samplers.cpp:75-93): all M rows in one
    // launch
    if (init) {
        std::vector<double> l0(M);
        const int rc = carma_mlogdensity_batch(h, init, s->series.data(), M, 0, l0.data());
        if (rc != CARMA_OK) return rc;
        for (int j = 0; j < M; j++) {
            if (!std::isfinite(l0[j])) continue;
            for (size_t k = j * per_run; k < (j + 1) * per_run; k++) {
                std::memcpy(&theta[k * d], init + (size_t)j * d, sizeof(double) * d);
                lp[k] = l0[j];
                done[k] = 1;
            }
        }
    }
    // Drawn starts: chain k = ladder T + temperature of the ENSEMBLE keys its generator, so run j draws what a single-series sampler
    // sharded to replica0 = j R draws; the candidates still pending of ALL runs are evaluated in one launch per round.
    std::vector<int> which;
    const int rc = find_starts(
        nchain, d, theta.data(), lp.data(), done.data(),
        [&](size_t k, int round, double* out) {
            const int sj = s->series[k / per_run];
            std::mt19937_64 rng = start_rng(s->seed, (uint64_t)k, round);
            draw_start(c->t.data() + c->hoff[sj], c->y.data() + c->hoff[sj], c->n[sj], c->pr[sj], c->p, c->q, rng, out);
        },
        [&](const double* cand, const size_t* idx, size_t m, double* out) {
            which.resize(m);
            for (size_t i = 0; i < m; i++) which[i] = s->series[idx[i] / per_run];
            return carma_mlogdensity_batch(h, cand, which.data(), (int)m, 0, out);
        });
    if (rc != CARMA_OK) return rc;
    for (size_t k = 0; k < nchain; k++)
        if (!done[k]) {
            set_error("carma_mpt_start: no finite starting value found for chain %zu of run %zu (series %d)", k % per_run, k / per_run,
                      s->series[k / per_run]);
            return CARMA_EINVAL;
        }
    return carma_mpt_set_chains(h, theta.data(), lp.data());
}

int carma_mpt_get_factor(carma_mctx* h, double* chol)
{
    MptState* s = mpt_state(h, "carma_mpt_get_factor", false);
    if (!s || !chol) return CARMA_EINVAL;
    Mctx* c = reinterpret_cast<Mctx*>(h);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = pt_ens_get_factor(s, c->d, c->stream, chol);
    if (e != hipSuccess) return hip_fail(e, "carma_mpt_get_factor");
    return CARMA_OK;
}

int carma_mpt_set_factor(carma_mctx* h, const double* chol)
{
    MptState* s = mpt_state(h, "carma_mpt_set_factor", false);
    if (!s || !chol) return CARMA_EINVAL;
    Mctx* c = reinterpret_cast<Mctx*>(h);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = pt_ens_set_factor(s, c->d, c->stream, chol);
    if (e != hipSuccess) return hip_fail(e, "carma_mpt_set_factor");
    return CARMA_OK;
}

int carma_mpt_iterate(carma_mctx* h, long niter, int do_exchange)
{
    MptState* s = mpt_state(h, "carma_mpt_iterate", true);
    if (!s) return CARMA_EINVAL;
    if (niter < 0) {
        set_error("carma_mpt_iterate: niter < 0");
        return CARMA_EINVAL;
    }
    Mctx* c = reinterpret_cast<Mctx*>(h);
    const hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    return mpt_iterate(c, niter, do_exchange, 0, nullptr);
}

int carma_mpt_sample(carma_mctx* h, int nsamples, int thin, double* samples, double* logposts)
{
    MptState* s = mpt_state(h, "carma_mpt_sample", true);
    if (!s) return CARMA_EINVAL;
    if (nsamples < 1 || thin < 1 || !samples || !logposts) {
        set_error("carma_mpt_sample: bad argument (nsamples >= 1, thin >= 1, non-null outputs)");
        return CARMA_EINVAL;
    }
    Mctx* c = reinterpret_cast<Mctx*>(h);
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    long capacity = 0;
    e = s->reserve_samples(c->d, nsamples, &capacity);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("carma_mpt_sample: no device memory for the sample buffer: %zu bytes asked for (%ld ladders x %d samples x %d)",
                  sizeof(double) * (size_t)s->R * nsamples * (c->d + 1), (long)s->R, nsamples, c->d);
        return CARMA_ENOMEM;
    }
    long off = 0;
    int rc = mpt_iterate(c, (long)nsamples * thin, 1, thin, &off);
    if (rc == CARMA_OK) {
        e = pt_ens_fetch_samples(s, c->d, nsamples, samples, logposts);
        if (e != hipSuccess) rc = hip_fail(e, "carma_mpt_sample: D2H");
    }
    s->cap = capacity;
    return rc;
}

int carma_mpt_stats(carma_mctx* h, double* accept_rate, double* swap_rate, int reset)
{
    MptState* s = mpt_state(h, "carma_mpt_stats", false);
    if (!s) return CARMA_EINVAL;
    Mctx* c = reinterpret_cast<Mctx*>(h);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = pt_ens_stats(s, accept_rate, swap_rate, reset);
    if (e != hipSuccess) return hip_fail(e, "carma_mpt_stats");
    return CARMA_OK;
}

long carma_mpt_iterations_done(const carma_mctx* h)
{
    if (!h || !reinterpret_cast<const Mctx*>(h)->mpt) return CARMA_EINVAL;
    return (long)reinterpret_cast<const Mctx*>(h)->mpt->iter;
}

int carma_mpt_logdensity(carma_mctx* h, const double* theta, double* out)
{
    MptState* s = mpt_state(h, "carma_mpt_logdensity", false);
    if (!s) return CARMA_EINVAL;
    if (!theta || !out) {
        set_error("carma_mpt_logdensity: null theta or out");
        return CARMA_EINVAL;
    }
    Mctx* c = reinterpret_cast<Mctx*>(h);
    const size_t nchain = s->nchain(), GUARD = 64;
    // [nc][d] proposals, [nc] results, then GUARD words nobody may write: a kernel whose idle lanes stored would show here
    std::vector<double> res(nchain + GUARD, 0.0);
    const double mark = -12345.678;
    std::fill(res.begin() + nchain, res.end(), mark);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = c->k_res.need(sizeof(double) * (nchain * c->d + nchain + GUARD));
    double *d_th = c->k_res.as<double>(), *d_ll = d_th + nchain * c->d;
    if (e == hipSuccess) e = hipMemcpyAsync(d_th, theta, sizeof(double) * nchain * c->d, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_ll, res.data(), sizeof(double) * res.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_logdens_chains_ms(c, s, d_th, (long)nchain, d_ll, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(res.data(), d_ll, sizeof(double) * res.size(), hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return hip_fail(e, "carma_mpt_logdensity");
    for (size_t k = nchain; k < res.size(); k++)
        if (res[k] != mark) {
            set_error("carma_mpt_logdensity: the kernel wrote past its %zu results", nchain);
            return CARMA_EHIP;
        }
    std::memcpy(out, res.data(), sizeof(double) * nchain);
    return CARMA_OK;
}

int carma_mpt_kernel_name(const carma_mctx* h, char* buf, int len)
{
    if (!h || !buf || len < 1) return CARMA_EINVAL;
    const Mctx* c = reinterpret_cast<const Mctx*>(h);
    const int r = c->p == 1 ? snprintf(buf, len, "k_logdens_car1_chains_ms") : snprintf(buf, len, "k_logdens_carma_chains_ms<%d>", c->p);
    return r > 0 ? CARMA_OK : CARMA_EINVAL;
}

int carma_mpt_run(carma_mctx* h, const int* series, int M, int ntemps, int nreplicas, int sample_size, int burnin, int thin,
                  const double* init, uint64_t seed, double* samples, double* logposts)
{
    int rc = carma_mpt_create(h, series, M, ntemps, nreplicas, nullptr, burnin, seed);
    if (rc == CARMA_OK) rc = carma_mpt_start(h, init);
    if (rc == CARMA_OK) rc = carma_mpt_iterate(h, burnin, 1);                     // Sampler::Run burn-in (samplers.cpp:97)
    if (rc == CARMA_OK) rc = carma_mpt_sample(h, sample_size, thin, samples, logposts);   // :101-108
    return rc;
}

}  // extern "C"
