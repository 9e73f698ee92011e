// carma_mband_set_pt.hip -- the SAMPLER over a set of multi-band objects (carma_bandset_pt_*):
// the large-ensemble sampler of carma_pt_lane.hip -- one chain per lane, an iteration as propose / K1 / finish -- on the extended
// vectors of MANY objects of a carma_bandset handle at once.  A RUN is one sampler (R replicas x T temperatures) on one object; a
// call's M runs are the ladders j R ... j R + R - 1 of ONE ensemble of M R ladders (as carma_mpt.hip), so the bookkeeping
// kernels, the Philox keys and the start-value keys are those of a single-object ensemble of that size: run j walks, bit for bit,
// what ladders j R ... of carma_bands_pt_* walk on a handle of its object alone.
// K1 is k_logdens_carma_mband_chains_ms: the body of k_logdens_carma_mband_chains with the object chosen per WAVE, as
// k_logdens_carma_mband_ms chooses it -- a wave never spans two runs (the wave map of carma_mband_set_pt_plan.h), so the band
// offsets in LDS, the trip count, the lag boxes and the prior stay wave-uniform.  The cost: a run of RT = R T chains takes
// ceil(RT / 64) waves of its own, and the default ladder (T = 10, R = 1) leaves 54 pad lanes in its wave.
// The host-only decisions are in carma_mband_set_pt_plan.h; what a run takes from its object (initial factor, default box,
// starting draw, box test) are the functions of carma_mband_pt_plan.h on that object's bands.
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
#include "carma_mband.h"
#include "carma_host.h"
#include "carma_mband_set_ctx.h"
#include "carma_mband_set_pt_plan.h"

namespace carma {

static_assert(MBANDSET_PT_LANES == MBAND_LANES, "the wave map and the kernels disagree on the lanes of a wave");

// K1 of the set sampler: ONE CHAIN PER LANE, a wave on ONE run.  Wave b = blockIdx.x serves run j = b / W (W = ceil(RT / 64)
// waves a run), chains j RT + 64 (b % W) + lane of the ensemble, on object run_obj[j]; thn = [M RT][dx] chain-major (the
// proposals the bookkeeping kernels write), ll = [M RT].  The body is logdensity_mband_lane with the prior: inside its run's box a
// chain gets the bits of k_logdens_carma_mband_chains on its object.  box = [M][2][K - 1][2], per run lo then hi of (log a_b,
// mu_b), or null: a chain with a band term outside (or NaN) gets -inf.  The lanes past the run's last chain shadow the wave's
// first chain and write nothing; lane 0 of every wave is live.
template <int P>
__global__ __launch_bounds__(64) void k_logdens_carma_mband_chains_ms(const double* __restrict__ thn, int dx, int q, int K, int RT,
                                                                     int W, const double4* __restrict__ rec,
                                                                     const long* __restrict__ off, const int* __restrict__ boff,
                                                                     const int* __restrict__ nobj, const double* __restrict__ lagbox,
                                                                     const Prior* __restrict__ prs, const int* __restrict__ run_obj,
                                                                     const double* __restrict__ box, double* __restrict__ ll)
{
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];   // all LDS is dynamic (mband_lds_bytes)
    const int lane = threadIdx.x;
    // wave-uniform: the run and everything of its object derive from blockIdx.x alone.  These loads stand ahead of the carve and
    // its barrier, where they stay scalar loads (k_logdens_carma_mband_ms)
    const int j = (int)(blockIdx.x / (unsigned)W), w = (int)(blockIdx.x - (unsigned)j * (unsigned)W);
    const int s = run_obj[j];
    const double4* orec = rec + off[s];
    const int N = nobj[s];
    const Prior pr = prs[s];
    const double* obox = lagbox + (long)s * 2 * (K - 1);
    const double* rbox = box ? box + (long)j * 4 * (K - 1) : nullptr;
    MbandWork wk;
    const double* s_tab = mband_lds_carve(s_dyn, K, K, lane, boff, s, wk);
    const int k0 = 64 * w;                                   // first chain of the wave within its run (< RT)
    const bool live = k0 + lane < RT;
    const long gi = (long)j * RT + k0 + (live ? lane : 0);
    const double* thx = thn + gi * dx;
    double v = logdensity_mband_lane<P>(thx, q, K, N, orec, obox, pr, 0, s_tab, wk);
    if (rbox) {
        const int d = dx - 3 * (K - 1), nb = 2 * (K - 1);
        bool in = true;
        for (int i = 0; i < nb; i++) {
            const double x = thx[d + 3 * (i >> 1) + 1 + (i & 1)];
            in = in && x >= rbox[i] && x <= rbox[nb + i];
        }
        if (!in) v = -1.0 / 0.0;
    }
    if (live) ll[gi] = v;
}

// K1 over the WHOLE ensemble of s: nc must be its M RT chains (the wave map knows no partial ensemble)
static hipError_t launch_logdens_mband_chains_ms(const BSctx* c, const BSptState* s, const double* thn, long nc, double* ll, hipStream_t st)
{
    (void)hipGetLastError();   // HIP's last-error is sticky: drop anything left by earlier calls
    const long RT = (long)s->reps * s->T;
    if (nc != (long)s->M * RT || nc <= 0) return hipErrorInvalidValue;
    const long W = mbandset_pt_run_waves(RT);
    const dim3 grid((unsigned)mbandset_pt_grid(s->M, RT)), block(64);
    const size_t lds = mband_lds_bytes(c->K);
    const double* box = s->has_box ? s->d_box.get() : nullptr;
    auto go = [&](auto P) {
        hipLaunchKernelGGL((k_logdens_carma_mband_chains_ms<decltype(P)::value>), grid, block, lds, st, thn, c->dx, c->q, c->K, (int)RT,
                           (int)W, c->d_rec.as<const double4>(), c->d_off.as<const long>(), c->d_boff.as<const int>(),
                           c->d_N.as<const int>(), c->d_lagbox.as<const double>(), c->d_pr.as<const Prior>(),
                           (const int*)s->d_run_obj.get(), box, ll);
        return hipGetLastError();
    };
    if (c->p == 1) return go(std::integral_constant<int, 1>{});   // (CAR(1) is the generic body at P = 1, as launch_logdens_mband)
    return for_order(c->p, hipErrorInvalidValue, go);
}

// the sampler state of h, or null with the error set: `who` was called before carma_bandset_pt_create (need_start: or before the
// chains have starting values)
static BSptState* bspt_state(carma_bandset* h, const char* who, bool need_start)
{
    if (!h) {
        set_error("%s: null context", who);
        return nullptr;
    }
    BSptState* s = reinterpret_cast<BSctx*>(h)->bspt.get();
    if (!s) {
        set_error("%s: call carma_bandset_pt_create first", who);
        return nullptr;
    }
    if (need_start && !s->started) {
        set_error("%s: chains have no starting values (carma_bandset_pt_start / carma_bandset_pt_set_chains)", who);
        return nullptr;
    }
    return s;
}

// the bands of object s as the functions of carma_mband_pt_plan.h take them
static std::vector<BandView> band_views(const BSctx* c, int s)
{
    std::vector<BandView> v((size_t)c->K);
    for (int b = 0; b < c->K; b++) {
        const size_t i = (size_t)s * c->K + b;
        v[b] = BandView{c->m.ts[i].data(), c->m.ys[i].data(), c->m.n[i]};
    }
    return v;
}

// The log-density the chains of the sampler have at thx [m][dx], row i a chain of run run[i]: the library's on the run's object,
// with the prior, and -inf outside the run's band box.  Rows outside their box never reach the device (all of them: no launch).
static int bspt_logdens_host(carma_bandset* h, const BSptState* s, const double* thx, const int* run, size_t m, double* out)
{
    BSctx* c = reinterpret_cast<BSctx*>(h);
    const size_t dx = (size_t)c->dx, nb = 2 * (size_t)(c->K - 1);
    std::vector<size_t> in;
    for (size_t i = 0; i < m; i++) {
        const double* bx = s->has_box ? s->box.data() + (size_t)run[i] * 2 * nb : nullptr;
        if (mband_pt_in_box(thx + i * dx, c->d, c->K, bx, bx ? bx + nb : nullptr))
            in.push_back(i);
        else
            out[i] = -std::numeric_limits<double>::infinity();
    }
    if (in.empty()) return CARMA_OK;
    std::vector<int> obj(in.size());
    for (size_t k = 0; k < in.size(); k++) obj[k] = s->run_obj[run[in[k]]];
    if (in.size() == m) return carma_bandset_logdensity_batch(h, thx, obj.data(), (int)m, 0, out);
    std::vector<double> sub(in.size() * dx), res(in.size());
    for (size_t k = 0; k < in.size(); k++) std::memcpy(&sub[k * dx], thx + in[k] * dx, sizeof(double) * dx);
    const int rc = carma_bandset_logdensity_batch(h, sub.data(), obj.data(), (int)in.size(), 0, res.data());
    if (rc != CARMA_OK) return rc;
    for (size_t k = 0; k < in.size(); k++) out[in[k]] = res[k];
    return CARMA_OK;
}

// niter iterations, a chunk in flight at a time.  thin > 0: save the coldest chains every thin iterations from sample *save_offset
// on.  The stream is idle when this returns, whatever happened.
static int bspt_iterate(BSctx* c, long niter, int do_exchange, int thin, long* save_offset)
{
    BSptState* s = c->bspt.get();
    const PtLaneK1 k1 = [c, s](const double* thn, long nc, double* ll, hipStream_t st) {
        return launch_logdens_mband_chains_ms(c, s, thn, nc, ll, st);
    };
    long left = niter;
    while (left > 0) {
        const long ch = pt_next_chunk(left, s->chunk0, thin);
        const PtLaunch L = pt_ens_launch(s, c->dx, c->q, s->nmax, ch, do_exchange, thin, save_offset ? *save_offset : 0);
        hipError_t e = launch_pt_lane_k1(c->p, L, s->d_scratch, k1, pt_ens_buffers(s), !s->factor_loaded, c->stream);
        if (e == hipSuccess) {
            s->factor_loaded = true;
            s->chol_stale = true;
        }
        const hipError_t es = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) return hip_fail(e, "carma_bandset_pt: sampler launch");
        pt_ens_advance(s, ch, thin, save_offset);
        left -= ch;
    }
    return CARMA_OK;
}

}  // namespace carma

using namespace carma;

extern "C" {

int carma_bandset_pt_default_box(const carma_bandset* h, int object, double* band_lo, double* band_hi)
{
    if (!h || !band_lo || !band_hi) {
        set_error("carma_bandset_pt_default_box: null context or output");
        return CARMA_EINVAL;
    }
    const BSctx* c = reinterpret_cast<const BSctx*>(h);
    if (object < 0 || object >= c->S) {
        set_error("carma_bandset_pt_default_box: object %d out of range (nobjects = %d)", object, c->S);
        return CARMA_EINVAL;
    }
    const std::vector<BandView> bands = band_views(c, object);
    mband_pt_default_box(bands.data(), c->K, band_lo, band_hi);
    return CARMA_OK;
}

int carma_bandset_pt_create(carma_bandset* h, const int* run_obj, int M, int ntemps, int nreplicas, const double* temperatures,
                            int adapt_iters, uint64_t seed, const double* band_lo, const double* band_hi)
{
    if (!h) {
        set_error("carma_bandset_pt_create: null context");
        return CARMA_EINVAL;
    }
    BSctx* c = reinterpret_cast<BSctx*>(h);
    const int K = c->K, dx = c->dx;
    std::vector<int> n0((size_t)c->S);
    for (int s = 0; s < c->S; s++) n0[s] = c->m.n[(size_t)s * K];
    const std::string bad = mbandset_pt_check_create(run_obj, M, c->S, ntemps, nreplicas, adapt_iters, dx, K, n0.data(), band_lo, band_hi);
    if (!bad.empty()) {
        set_error("carma_bandset_pt_create: %s", bad.c_str());
        return CARMA_EINVAL;
    }
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    c->bspt.reset(new BSptState());       // (the state of an earlier call goes, with every buffer it holds)
    BSptState* s = c->bspt.get();
    s->M = M;
    s->reps = nreplicas;
    s->maxiter = adapt_iters;
    s->seed = seed;
    s->run_obj.assign(run_obj, run_obj + M);
    s->chunk0 = mbandset_pt_chunk_iters(run_obj, M, c->m.N.data());
    for (int j = 0; j < M; j++) s->nmax = std::max(s->nmax, c->m.N[run_obj[j]]);
    std::vector<double> temps;
    default_ladder(ntemps, temperatures, temps);             // shared by all runs
    const size_t per_run = (size_t)nreplicas * ntemps, nchain = (size_t)M * per_run, nb = 2 * (size_t)(K - 1);
    // initial proposal factor of run j, from ITS object
    std::vector<double> chol(nchain * dx * dx), R0((size_t)dx * dx);
    for (int j = 0; j < M; j++) {
        const std::vector<BandView> bands = band_views(c, run_obj[j]);
        mband_pt_initial_factor(bands.data(), K, c->d, R0.data());
        for (size_t k = j * per_run; k < (j + 1) * per_run; k++) std::memcpy(&chol[k * dx * dx], R0.data(), sizeof(double) * dx * dx);
    }
    s->has_box = band_lo != nullptr && nb > 0;
    if (s->has_box)
        for (int j = 0; j < M; j++) {                        // [M][2][K - 1][2]: a run's lo then its hi
            s->box.insert(s->box.end(), band_lo + (size_t)j * nb, band_lo + (size_t)(j + 1) * nb);
            s->box.insert(s->box.end(), band_hi + (size_t)j * nb, band_hi + (size_t)(j + 1) * nb);
        }
    e = pt_ens_create(s, ntemps, M * nreplicas, dx, temps, chol.data());
    if (e == hipSuccess) e = s->d_scratch.alloc(pt_lane_scratch_doubles(dx, (long)nchain));
    if (e == hipSuccess) e = s->d_run_obj.alloc((size_t)M);
    if (e == hipSuccess) e = hipMemcpy(s->d_run_obj, s->run_obj.data(), sizeof(int) * (size_t)M, hipMemcpyHostToDevice);
    if (e == hipSuccess && s->has_box) e = s->d_box.alloc(s->box.size());
    if (e == hipSuccess && s->has_box) e = hipMemcpy(s->d_box, s->box.data(), sizeof(double) * s->box.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        c->bspt.reset();
        return hip_fail(e, "carma_bandset_pt_create");
    }
    return CARMA_OK;
}

int carma_bandset_pt_set_chains(carma_bandset* h, const double* theta, const double* logpost)
{
    BSptState* s = bspt_state(h, "carma_bandset_pt_set_chains", false);
    if (!s) return CARMA_EINVAL;
    if (!theta) {
        set_error("carma_bandset_pt_set_chains: null theta");
        return CARMA_EINVAL;
    }
    BSctx* c = reinterpret_cast<BSctx*>(h);
    const size_t nchain = s->nchain(), per_run = (size_t)s->reps * s->T;
    std::vector<double> lp(nchain);
    if (logpost) {
        std::memcpy(lp.data(), logpost, sizeof(double) * nchain);
    } else {
        std::vector<int> run(nchain);
        for (size_t k = 0; k < nchain; k++) run[k] = (int)(k / per_run);
        const int rc = bspt_logdens_host(h, s, theta, run.data(), nchain, lp.data());
        if (rc != CARMA_OK) return rc;
    }
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = pt_ens_set_chains(s, c->dx, theta, lp.data());
    if (e != hipSuccess) return hip_fail(e, "carma_bandset_pt_set_chains");
    s->started = true;
    return CARMA_OK;
}

int carma_bandset_pt_get_chains(carma_bandset* h, double* theta, double* logpost)
{
    BSptState* s = bspt_state(h, "carma_bandset_pt_get_chains", false);
    if (!s) return CARMA_EINVAL;
    BSctx* c = reinterpret_cast<BSctx*>(h);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = pt_ens_get_chains(s, c->dx, theta, logpost);
    if (e != hipSuccess) return hip_fail(e, "carma_bandset_pt_get_chains");
    return CARMA_OK;
}

int carma_bandset_pt_start(carma_bandset* h, const double* init)
{
    BSptState* s = bspt_state(h, "carma_bandset_pt_start", false);
    if (!s) return CARMA_EINVAL;
    BSctx* c = reinterpret_cast<BSctx*>(h);
    const int dx = c->dx, M = s->M;
    const size_t per_run = (size_t)s->reps * s->T, nchain = s->nchain();
    std::vector<double> theta(nchain * dx), lp(nchain, -std::numeric_limits<double>::infinity());
    std::vector<char> done(nchain, 0);
    std::vector<int> run;
    // a run's init row is honoured when its log-density on the run's object is finite (and inside the run's box): it becomes
    // every chain of that run; all M rows in one launch
    if (init) {
        std::vector<double> l0((size_t)M);
        run.resize((size_t)M);
        for (int j = 0; j < M; j++) run[j] = j;
        const int rc = bspt_logdens_host(h, s, init, run.data(), (size_t)M, l0.data());
        if (rc != CARMA_OK) return rc;
        for (int j = 0; j < M; j++) {
            if (!std::isfinite(l0[j])) continue;
            for (size_t k = j * per_run; k < (j + 1) * per_run; k++) {
                std::memcpy(&theta[k * dx], init + (size_t)j * dx, sizeof(double) * dx);
                lp[k] = l0[j];
                done[k] = 1;
            }
        }
    }
    // Drawn starts: chain k = ladder T + temperature of the ENSEMBLE keys its generator, so run j draws what carma_bands_pt_start
    // draws for ladders j R ... on a handle of its object; the candidates still pending of ALL runs are evaluated in one launch
    // per round.
    std::vector<std::vector<BandView>> views((size_t)M);
    for (int j = 0; j < M; j++) views[j] = band_views(c, s->run_obj[j]);
    const int rc = find_starts(
        nchain, dx, theta.data(), lp.data(), done.data(),
        [&](size_t k, int round, double* out) {
            const size_t j = k / per_run;
            const int sj = s->run_obj[j];
            mband_pt_draw_start(views[j].data(), c->K, c->m.pr[sj], c->p, c->q, c->m.lagbox.data() + (size_t)sj * 2 * (c->K - 1), s->seed,
                                (uint64_t)k, round, out);
        },
        [&](const double* cand, const size_t* idx, size_t m, double* out) {
            run.resize(m);
            for (size_t i = 0; i < m; i++) run[i] = (int)(idx[i] / per_run);
            return bspt_logdens_host(h, s, cand, run.data(), m, out);
        });
    if (rc != CARMA_OK) return rc;
    for (size_t k = 0; k < nchain; k++)
        if (!done[k]) {
            set_error("carma_bandset_pt_start: no finite starting value found for chain %zu of run %zu (object %d)", k % per_run,
                      k / per_run, s->run_obj[k / per_run]);
            return CARMA_EINVAL;
        }
    return carma_bandset_pt_set_chains(h, theta.data(), lp.data());
}

int carma_bandset_pt_get_factor(carma_bandset* h, double* chol)
{
    BSptState* s = bspt_state(h, "carma_bandset_pt_get_factor", false);
    if (!s) return CARMA_EINVAL;
    if (!chol) {
        set_error("carma_bandset_pt_get_factor: null chol");
        return CARMA_EINVAL;
    }
    BSctx* c = reinterpret_cast<BSctx*>(h);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = pt_ens_get_factor(s, c->dx, c->stream, chol);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        return hip_fail(e, "carma_bandset_pt_get_factor");
    }
    return CARMA_OK;
}

int carma_bandset_pt_set_factor(carma_bandset* h, const double* chol)
{
    BSptState* s = bspt_state(h, "carma_bandset_pt_set_factor", false);
    if (!s) return CARMA_EINVAL;
    if (!chol) {
        set_error("carma_bandset_pt_set_factor: null chol");
        return CARMA_EINVAL;
    }
    BSctx* c = reinterpret_cast<BSctx*>(h);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = pt_ens_set_factor(s, c->dx, c->stream, chol);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        return hip_fail(e, "carma_bandset_pt_set_factor");
    }
    return CARMA_OK;
}

int carma_bandset_pt_iterate(carma_bandset* h, long niter, int do_exchange)
{
    BSptState* s = bspt_state(h, "carma_bandset_pt_iterate", true);
    if (!s) return CARMA_EINVAL;
    if (niter < 0) {
        set_error("carma_bandset_pt_iterate: niter < 0");
        return CARMA_EINVAL;
    }
    BSctx* c = reinterpret_cast<BSctx*>(h);
    const hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    return bspt_iterate(c, niter, do_exchange, 0, nullptr);
}

int carma_bandset_pt_sample(carma_bandset* h, int nsamples, int thin, double* samples, double* logposts)
{
    BSptState* s = bspt_state(h, "carma_bandset_pt_sample", true);
    if (!s) return CARMA_EINVAL;
    if (nsamples < 1 || thin < 1 || !samples || !logposts) {
        set_error("carma_bandset_pt_sample: bad argument (nsamples >= 1, thin >= 1, non-null outputs)");
        return CARMA_EINVAL;
    }
    BSctx* c = reinterpret_cast<BSctx*>(h);
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    long capacity = 0;
    e = s->reserve_samples(c->dx, nsamples, &capacity);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("carma_bandset_pt_sample: no device memory for the sample buffer: %zu bytes asked for (%ld ladders x %d samples x %d)",
                  sizeof(double) * (size_t)s->R * nsamples * (c->dx + 1), (long)s->R, nsamples, c->dx);
        return CARMA_ENOMEM;
    }
    long off = 0;
    int rc = bspt_iterate(c, (long)nsamples * thin, 1, thin, &off);
    if (rc == CARMA_OK) {
        e = pt_ens_fetch_samples(s, c->dx, nsamples, samples, logposts);
        if (e != hipSuccess) rc = hip_fail(e, "carma_bandset_pt_sample: D2H");
    }
    s->cap = capacity;
    return rc;
}

int carma_bandset_pt_stats(carma_bandset* h, double* accept_rate, double* swap_rate, int reset)
{
    BSptState* s = bspt_state(h, "carma_bandset_pt_stats", false);
    if (!s) return CARMA_EINVAL;
    BSctx* c = reinterpret_cast<BSctx*>(h);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = pt_ens_stats(s, accept_rate, swap_rate, reset);
    if (e != hipSuccess) return hip_fail(e, "carma_bandset_pt_stats");
    return CARMA_OK;
}

long carma_bandset_pt_iterations_done(const carma_bandset* h)
{
    if (!h || !reinterpret_cast<const BSctx*>(h)->bspt) return CARMA_EINVAL;
    return (long)reinterpret_cast<const BSctx*>(h)->bspt->iter;
}

int carma_bandset_pt_logdensity(carma_bandset* h, const double* theta, double* out)
{
    BSptState* s = bspt_state(h, "carma_bandset_pt_logdensity", false);
    if (!s) return CARMA_EINVAL;
    if (!theta || !out) {
        set_error("carma_bandset_pt_logdensity: null theta or out");
        return CARMA_EINVAL;
    }
    BSctx* c = reinterpret_cast<BSctx*>(h);
    const size_t nchain = s->nchain(), GUARD = 64;
    // [nc][dx] proposals, [nc] results, then GUARD words nobody may write: a kernel whose pad lanes stored would show here
    std::vector<double> res(nchain + GUARD, 0.0);
    const double mark = -12345.678;
    std::fill(res.begin() + nchain, res.end(), mark);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = s->k_res.need(sizeof(double) * (nchain * c->dx + nchain + GUARD));
    double *d_th = s->k_res.as<double>(), *d_ll = d_th + nchain * c->dx;
    if (e == hipSuccess) e = hipMemcpyAsync(d_th, theta, sizeof(double) * nchain * c->dx, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_ll, res.data(), sizeof(double) * res.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_logdens_mband_chains_ms(c, s, d_th, (long)nchain, d_ll, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(res.data(), d_ll, sizeof(double) * res.size(), hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return hip_fail(e, "carma_bandset_pt_logdensity");
    for (size_t k = nchain; k < res.size(); k++)
        if (res[k] != mark) {
            set_error("carma_bandset_pt_logdensity: the kernel wrote past its %zu results", nchain);
            return CARMA_EHIP;
        }
    std::memcpy(out, res.data(), sizeof(double) * nchain);
    return CARMA_OK;
}

int carma_bandset_pt_kernel_name(const carma_bandset* h, char* buf, int len)
{
    if (!h || !buf || len < 1) return CARMA_EINVAL;
    const BSctx* c = reinterpret_cast<const BSctx*>(h);
    return snprintf(buf, len, "k_logdens_carma_mband_chains_ms<%d>", c->p) > 0 ? CARMA_OK : CARMA_EINVAL;
}

int carma_bandset_pt_run(carma_bandset* h, const int* run_obj, int M, int ntemps, int nreplicas, int sample_size, int burnin, int thin,
                         const double* init, uint64_t seed, const double* band_lo, const double* band_hi, double* samples,
                         double* logposts)
{
    int rc = carma_bandset_pt_create(h, run_obj, M, ntemps, nreplicas, nullptr, burnin, seed, band_lo, band_hi);
    if (rc == CARMA_OK) rc = carma_bandset_pt_start(h, init);
    if (rc == CARMA_OK) rc = carma_bandset_pt_iterate(h, burnin, 1);                     // Sampler::Run burn-in (samplers.cpp:97)
    if (rc == CARMA_OK) rc = carma_bandset_pt_sample(h, sample_size, thin, samples, logposts);   // :101-108
    return rc;
}

}  // extern "C"
