// carma_mpt.hip -- the SAMPLER over many series (carma_mpt_*) of a multi-series context
// (carma_mseries.hip): the large-ensemble sampler of carma_pt_lane.hip -- one chain per
// lane, an iteration as k_ram_propose / K1 / k_ram_finish -- with a K1 in which every chain is evaluated on the series of its own
// ladder (k_logdens_carma_chains_ms).  A RUN is one sampler (R replicas x T temperatures) on one series; a call's M runs are the
// ladders j R .. j R + R - 1 of ONE ensemble of M R ladders, so the bookkeeping kernels, the Philox keys and the start-value keys
// are those of a single-series ensemble of that size, and run j is its block replica0 = j R.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "grp_device.h"
#include "carma_core.h"
#include "carma_lane.h"
#include "carma_mseries.h"
#include "carma_pt_front.h"

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

// The sampler of h as the shared front drives it (carma_pt_front.h).  A row is evaluated by carma_mlogdensity_batch on the series of
// its chain's run; chain k draws from ITS series with the generator its slot in the ensemble keys.
static PtFront mpt_front(carma_mctx* h)
{
    PtFront f;
    f.name = "carma_mpt";
    if (!h) return f;
    Mctx* c = reinterpret_cast<Mctx*>(h);
    MptState* s = c->mpt.get();
    f.has_ctx = true;
    f.device = c->device;
    f.stream = c->stream;
    f.p = c->p;
    f.q = c->q;
    f.dim = c->d;
    f.s = s;
    f.guard = &c->k_res;
    if (!s) return f;
    const size_t per_run = (size_t)s->reps * s->T;
    f.M = (size_t)s->M;
    f.per_run = per_run;
    f.n = s->nmax;
    f.chunk0 = s->chunk0;
    f.k1 = [c, s](const double* thn, long nc, double* ll, hipStream_t st) { return launch_logdens_chains_ms(c, s, thn, nc, ll, st); };
    f.eval = [h, s, per_run](const double* rows, const size_t* chain, size_t m, double* out) {
        std::vector<int> which(m);
        for (size_t i = 0; i < m; i++) which[i] = s->series[(chain ? chain[i] : i) / per_run];
        return carma_mlogdensity_batch(h, rows, which.data(), (int)m, 0, out);
    };
    f.draw = [c, s, per_run](size_t k, int round, double* out) {
        const int sj = s->series[k / per_run];
        std::mt19937_64 rng = start_rng(s->seed, (uint64_t)k, round);
        draw_start(c->t.data() + c->hoff[sj], c->y.data() + c->hoff[sj], c->n[sj], c->pr[sj], c->p, c->q, rng, out);
    };
    f.which = [s, per_run](size_t k) {
        char buf[96];
        snprintf(buf, sizeof(buf), "chain %zu of run %zu (series %d)", k % per_run, k / per_run, s->series[k / per_run]);
        return std::string(buf);
    };
    return f;
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
    s->chunk0 = mpt_chunk_iters(s->nmax);
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
    return pt_front_set_chains(mpt_front(h), theta, logpost);
}

int carma_mpt_get_chains(carma_mctx* h, double* theta, double* logpost) { return pt_front_get_chains(mpt_front(h), theta, logpost); }

int carma_mpt_start(carma_mctx* h, const double* init) { return pt_front_start(mpt_front(h), init); }

int carma_mpt_get_factor(carma_mctx* h, double* chol) { return pt_front_get_factor(mpt_front(h), chol); }

int carma_mpt_set_factor(carma_mctx* h, const double* chol) { return pt_front_set_factor(mpt_front(h), chol); }

int carma_mpt_iterate(carma_mctx* h, long niter, int do_exchange) { return pt_front_iterate(mpt_front(h), niter, do_exchange); }

int carma_mpt_sample(carma_mctx* h, int nsamples, int thin, double* samples, double* logposts)
{
    return pt_front_sample(mpt_front(h), nsamples, thin, samples, logposts);
}

int carma_mpt_stats(carma_mctx* h, double* accept_rate, double* swap_rate, int reset)
{
    return pt_front_stats(mpt_front(h), accept_rate, swap_rate, reset);
}

long carma_mpt_iterations_done(const carma_mctx* h) { return pt_front_iterations_done(mpt_front(const_cast<carma_mctx*>(h))); }

int carma_mpt_logdensity(carma_mctx* h, const double* theta, double* out) { return pt_front_logdensity(mpt_front(h), theta, out); }

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
    const int rc = carma_mpt_create(h, series, M, ntemps, nreplicas, nullptr, burnin, seed);
    return rc == CARMA_OK ? pt_front_run(mpt_front(h), init, burnin, sample_size, thin, samples, logposts) : rc;
}

}  // extern "C"
