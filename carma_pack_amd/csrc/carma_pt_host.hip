// carma_pt_host.hip -- host side of the parallel-tempering sampler behind the C ABI:
// temperature ladder, initial proposal covariance, starting values, chunked launches of the
// persistent kernel (carma_pt.hip), sample collection.
// Reference: RunCarmaSampler / RunCar1Sampler (src/carmcmc.cpp:30-177), Sampler::Run
// (src/samplers.cpp:57-115), StartingValue routines (src/carpack.cpp:38-81,175-230,268-311,416-477).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../include/carma_mi355.h"
#include "carma_host.h"
#include "carma_pt_sched.h"

namespace carma {

// ---- the ensemble both samplers hold (PtEnsemble, carma_pt_state.h) --------------------------------------------------------------
hipError_t pt_ens_create(PtEnsemble* s, int T, int R, int d, const std::vector<double>& temps, const double* chol)
{
    s->temps = temps;
    hipError_t e = s->reserve(T, R, d);
    const size_t nchain = s->nchain();
    if (e == hipSuccess) e = hipMemcpy(s->d_temps, s->temps.data(), sizeof(double) * T, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_chol, chol, sizeof(double) * nchain * d * d, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(s->d_nacc, 0, sizeof(unsigned) * nchain);
    if (e == hipSuccess) e = hipMemset(s->d_nswap, 0, sizeof(unsigned) * nchain);
    return e;
}

PtLaunch pt_ens_launch(const PtEnsemble* s, int d, int q, int n, long ch, int do_exchange, int thin, long save_offset)
{
    PtLaunch L{};
    L.d = d;
    L.q = q;
    L.n = n;
    L.T = s->T;
    L.R = s->R;
    L.maxiter = s->maxiter;
    L.iter0 = s->iter;
    L.niter = (int)ch;
    L.do_exchange = do_exchange;
    L.save_thin = thin;
    L.save_offset = save_offset;
    L.sample_cap = s->cap;
    L.seed0 = (unsigned)(s->seed & 0xffffffffu);
    L.seed1 = (unsigned)(s->seed >> 32);
    L.slot0 = 0;
    L.T_global = (unsigned)s->T;
    L.replica0 = 0;
    return L;
}

void pt_ens_advance(PtEnsemble* s, long ch, int thin, long* save_offset)
{
    s->iter += ch;
    s->stat_iters += ch;
    if (thin > 0 && save_offset) *save_offset += ch / thin;
}

hipError_t pt_ens_set_chains(PtEnsemble* s, int d, const double* theta, const double* lp)
{
    hipError_t e = hipMemcpy(s->d_theta, theta, sizeof(double) * s->nchain() * d, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_lp, lp, sizeof(double) * s->nchain(), hipMemcpyHostToDevice);
    return e;
}

hipError_t pt_ens_get_chains(const PtEnsemble* s, int d, double* theta, double* lp)
{
    hipError_t e = hipSuccess;
    if (theta) e = hipMemcpy(theta, s->d_theta, sizeof(double) * s->nchain() * d, hipMemcpyDeviceToHost);
    if (e == hipSuccess && lp) e = hipMemcpy(lp, s->d_lp, sizeof(double) * s->nchain(), hipMemcpyDeviceToHost);
    return e;
}

hipError_t pt_ens_fetch_samples(const PtEnsemble* s, int d, int nsamples, double* samples, double* logposts)
{
    hipError_t e = hipMemcpy(samples, s->d_samples, sizeof(double) * (size_t)s->R * nsamples * d, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(logposts, s->d_slp, sizeof(double) * (size_t)s->R * nsamples, hipMemcpyDeviceToHost);
    return e;
}

hipError_t pt_ens_stats(PtEnsemble* s, double* accept_rate, double* swap_rate, int reset)
{
    const size_t nchain = s->nchain();
    std::vector<unsigned> a(nchain), w(nchain);
    hipError_t e = hipMemcpy(a.data(), s->d_nacc, sizeof(unsigned) * nchain, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(w.data(), s->d_nswap, sizeof(unsigned) * nchain, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    const double it = s->stat_iters ? (double)s->stat_iters : 1.0;
    for (size_t k = 0; k < nchain; k++) {
        if (accept_rate) accept_rate[k] = a[k] / it;
        if (swap_rate) swap_rate[k] = w[k] / it;   // entry i = swaps between temperature i and i-1
    }
    if (reset) {
        (void)hipMemset(s->d_nacc, 0, sizeof(unsigned) * nchain);
        (void)hipMemset(s->d_nswap, 0, sizeof(unsigned) * nchain);
        s->stat_iters = 0;
    }
    return hipSuccess;
}

hipError_t pt_ens_sync_factor(PtEnsemble* s, int d, hipStream_t st)
{
    if (!s->chol_stale) return hipSuccess;
    const hipError_t e = pt_lane_store_factor(d, s->T, s->R, s->d_scratch, s->d_chol, st);
    if (e == hipSuccess) s->chol_stale = false;
    return e;
}

void pt_ens_factor_written(PtEnsemble* s)
{
    s->factor_loaded = false;
    s->chol_stale = false;
}

hipError_t pt_ens_get_factor(PtEnsemble* s, int d, hipStream_t st, double* chol)
{
    hipError_t e = pt_ens_sync_factor(s, d, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(chol, s->d_chol, sizeof(double) * s->nchain() * d * d, hipMemcpyDeviceToHost);
    return e;
}

hipError_t pt_ens_set_factor(PtEnsemble* s, int d, hipStream_t st, const double* chol)
{
    hipError_t e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(s->d_chol, chol, sizeof(double) * s->nchain() * d * d, hipMemcpyHostToDevice);
    if (e == hipSuccess) pt_ens_factor_written(s);
    return e;
}

static int chunk_iters(const Ctx* c)
{
    // Iterations per launch.  Ladder kernel: around a quarter of a second (~0.8 us per datum per iteration for p >= 5).
    // Row kernel: ~0.14 us per datum per iteration, and its COOPERATIVE launch costs ~2 ms on this stack -- 4.5 % of a
    // 44 ms chunk (measured) -- so its chunks are sized for half a second.
    if (c->pt && c->pt->use_row) {
        const double est_us = std::max(1.0, 0.14 * c->n);
        return (int)std::max(1.0, std::min(16384.0, 500000.0 / est_us));
    }
    if (c->pt && c->pt->use_lane) {                       // large ensembles: >= ~0.45 us per datum per iteration, 2 launches each
        const double est_us = std::max(1.0, 0.45 * c->n);
        return (int)std::max(1.0, std::min(4096.0, 250000.0 / est_us));
    }
    const double est_us = std::max(1.0, 0.8 * c->n * (c->p >= 5 ? 1.0 : 0.5));
    return (int)std::max(1.0, std::min(4096.0, 250000.0 / est_us));
}

// one launch of `ch` iterations on `st`
static int pt_enqueue_one(Ctx* c, long ch, int do_exchange, int thin, long* save_offset, hipStream_t st)
{
    PtState* s = c->pt.get();
    PtLaunch L = pt_ens_launch(s, c->d, c->q, c->n, ch, do_exchange, thin, save_offset ? *save_offset : 0);
    L.slot0 = s->slot0;                                     // this context's block of the ladder and of the replicas (carma_pt_shard)
    L.T_global = s->T_global;
    L.replica0 = s->replica0;
    hipError_t e;
    if (s->use_row) {
        PtRowSync S{s->d_stage, s->d_abort, ++s->epoch, s->wpl, device_cus(), 1, c->series_flags(), 0};
        e = launch_pt_row(c->p, L, S, c->rec(), c->pr, pt_ens_buffers(s), st);
        if (e == hipErrorCooperativeLaunchTooLarge) {      // the grid is not co-resident on this device: ladder kernel
            (void)hipGetLastError();
            s->use_row = false;
        }
    }
    if (!s->use_row && s->use_lane) {
        e = launch_pt_lane(c->p, L, s->d_scratch, c->rec(), c->pr, pt_ens_buffers(s), c->series_flags(), !s->factor_loaded, st);
        if (e == hipSuccess) {
            s->factor_loaded = true;                   // ... and stays in the scratch: the chain-major copy is behind until
            s->chol_stale = true;                           // somebody asks for it (pt_ens_sync_factor)
        }
    } else if (!s->use_row) {
        e = launch_pt(c->p, L, c->rec(), c->pr, pt_ens_buffers(s), st);
    }
    if (e != hipSuccess) return hip_fail(e, "launch pt kernel");
    pt_ens_advance(s, ch, thin, save_offset);
    return CARMA_OK;
}

int pt_enqueue(Ctx* c, long niter, int do_exchange, int thin, long* save_offset, hipStream_t st)
{
    const int chunk0 = chunk_iters(c);
    long left = niter;
    while (left > 0) {
        const long ch = pt_next_chunk(left, chunk0, thin);
        int rc = pt_enqueue_one(c, ch, do_exchange, thin, save_offset, st);
        if (rc != CARMA_OK) return rc;
        left -= ch;
    }
    return CARMA_OK;
}

int pt_check_abort(Ctx* c, bool* aborted)
{
    PtState* s = c->pt.get();
    *aborted = false;
    if (!s->use_row) return CARMA_OK;
    unsigned flag = 0;
    hipError_t e = hipMemcpy(&flag, s->d_abort, sizeof(unsigned), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "pt abort flag");
    *aborted = flag != 0;
    return CARMA_OK;
}

// chain state <-> backup (theta, logpost, chol), asynchronous on st
static hipError_t pt_backup(Ctx* c, bool restore, hipStream_t st)
{
    PtState* s = c->pt.get();
    const size_t nchain = (size_t)s->T * s->R, d = c->d;
    double* b = s->d_backup;
    struct Part { double* p; size_t n; } parts[3] = {{s->d_theta, nchain * d}, {s->d_lp, nchain}, {s->d_chol, nchain * d * d}};
    if (!restore) {
        const hipError_t es = pt_ens_sync_factor(s, c->d, st);
        if (es != hipSuccess) return es;
    } else {
        pt_ens_factor_written(s);
    }
    for (auto& pt : parts) {
        hipError_t e = restore ? hipMemcpyAsync(pt.p, b, sizeof(double) * pt.n, hipMemcpyDeviceToDevice, st)
                               : hipMemcpyAsync(b, pt.p, sizeof(double) * pt.n, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return e;
        b += pt.n;
    }
    return hipSuccess;
}

// Run `niter` iterations and wait for them.  The ladder kernel's launches are all enqueued first; the row kernel
// (cross-workgroup rendezvous) is run chunk by chunk with the chain state saved in front of every chunk: should a
// rendezvous ever time out (the launch is cooperative, so the grid is co-resident by construction; the time-out only
// guards against a wedged GPU), the chunk is restored and re-run -- like everything after it -- with the ladder kernel.
static int pt_launch_chunks(Ctx* c, long niter, int do_exchange, int thin, long* save_offset)
{
    PtState* s = c->pt.get();
    if (!s->use_row) {
        int rc = pt_enqueue(c, niter, do_exchange, thin, save_offset, c->stream);
        if (rc != CARMA_OK) return rc;
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return hip_fail(e, "pt kernel");
        return CARMA_OK;
    }
    const int chunk0 = chunk_iters(c);
    long left = niter;
    while (left > 0) {
        const long ch = pt_next_chunk(left, chunk0, thin);
        if (!s->use_row) return pt_launch_chunks(c, left, do_exchange, thin, save_offset);     // after a fall-back
        const unsigned long long iter_before = s->iter, stat_before = s->stat_iters;
        const long off_before = save_offset ? *save_offset : 0;
        hipError_t e = pt_backup(c, false, c->stream);
        if (e != hipSuccess) return hip_fail(e, "pt state backup");
        int rc = pt_enqueue_one(c, ch, do_exchange, thin, save_offset, c->stream);
        if (rc != CARMA_OK) return rc;
        e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return hip_fail(e, "pt kernel");
        bool aborted = false;
        rc = pt_check_abort(c, &aborted);
        if (rc != CARMA_OK) return rc;
        if (aborted) {
            e = pt_backup(c, true, c->stream);
            if (e == hipSuccess) e = hipMemsetAsync(s->d_abort, 0, sizeof(unsigned), c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) return hip_fail(e, "pt state restore");
            s->iter = iter_before;
            s->stat_iters = stat_before;
            if (save_offset) *save_offset = off_before;
            s->use_row = false;           // acceptance / swap counters of the aborted chunk stay counted: statistics only
            continue;
        }
        left -= ch;
    }
    return CARMA_OK;
}

}  // namespace carma

using namespace carma;

extern "C" {

int carma_pt_create(carma_ctx* h, int ntemps, int nreplicas, const double* temperatures, int adapt_iters, uint64_t seed)
{
    if (!h || ntemps < 1 || nreplicas < 1 || adapt_iters < 0) {
        set_error("carma_pt_create: bad argument");
        return CARMA_EINVAL;
    }
    Ctx* c = reinterpret_cast<Ctx*>(h);
    int nthr = 0;
    const size_t lds = pt_lds_bytes(c->p, c->d, ntemps, &nthr);
    if (nthr > 1024 || lds > 160 * 1024) {
        set_error("carma_pt_create: %d temperatures do not fit one workgroup (threads %d, LDS %zu B)", ntemps, nthr, lds);
        return CARMA_EINVAL;
    }
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    c->pt.reset(new PtState());           // (the state of an earlier call goes, with every buffer it holds)
    PtState* s = c->pt.get();
    s->T_global = ntemps;
    s->maxiter = adapt_iters;
    s->seed = seed;
    std::vector<double> temps;
    default_ladder(ntemps, temperatures, temps);
    const int d = c->d;
    const size_t nchain = (size_t)ntemps * nreplicas;
    std::vector<double> R0((size_t)d * d);
    initial_factor(pop_var(c->y.data(), c->n), c->n, d, R0.data());
    std::vector<double> chol(nchain * d * d);
    for (size_t k = 0; k < nchain; k++) std::memcpy(&chol[k * d * d], R0.data(), sizeof(double) * d * d);
    e = pt_ens_create(s, ntemps, nreplicas, d, temps, chol.data());
    // Kernel choice: pt_family (carma_shape_plan.h).  CARMA_PT_KERNEL=ladder|row|lane and CARMA_TUNE_PT_LANE_MIN are read HERE, at
    // every creation (callers set them between creations), and nowhere else.
    if (e == hipSuccess) {
        const char* force = getenv("CARMA_PT_KERNEL");
        const char* tv = getenv("CARMA_TUNE_PT_LANE_MIN");
        const PtForce forced = !force ? PtForce::NONE : !std::strcmp(force, "lane") ? PtForce::LANE : !std::strcmp(force, "ladder") ? PtForce::LADDER : PtForce::ROW;
        DeviceFacts f;
        f.cus = device_cus();
        f.row_per_cu = pt_row_per_cu(c->p, d, ntemps);
        const PtFamily fam = pt_family(c->p, ntemps, nreplicas, c->n, f, shape_switches(), forced, tv ? atol(tv) : TUNE_UNSET);
        if (fam == PtFamily::LANE) {
            s->use_lane = true;
            e = s->d_scratch.alloc(pt_lane_scratch_doubles(d, (long)nchain));
        } else if (fam == PtFamily::ROW) {
            s->use_row = true;
            s->wpl = (ntemps + 3) / 4;
            // the tagged staging is zeroed once (an all-zero pair of words never validates)
            e = s->reserve_row(d);
            if (e == hipSuccess) e = hipMemset(s->d_stage, 0, sizeof(unsigned long long) * 4 * nchain * (d + 1));
            if (e == hipSuccess) e = hipMemset(s->d_abort, 0, sizeof(unsigned));
        }
    }
    if (e != hipSuccess) {
        c->pt.reset();
        return hip_fail(e, "carma_pt_create");
    }
    return CARMA_OK;
}

int carma_pt_shard(carma_ctx* h, int ntemps_global, int slot0, int replica0)
{
    if (!h || !reinterpret_cast<Ctx*>(h)->pt) return CARMA_EINVAL;
    PtState* s = reinterpret_cast<Ctx*>(h)->pt.get();
    if (ntemps_global < s->T || slot0 < 0 || slot0 + s->T > ntemps_global || replica0 < 0) {
        set_error("carma_pt_shard: bad shard");
        return CARMA_EINVAL;
    }
    s->T_global = (unsigned)ntemps_global;
    s->slot0 = (unsigned)slot0;
    s->replica0 = (unsigned)replica0;
    return CARMA_OK;
}

int carma_pt_bind_state(carma_ctx* h, double* d_theta, double* d_logpost)
{
    if (!h || !reinterpret_cast<Ctx*>(h)->pt || !d_theta || !d_logpost) return CARMA_EINVAL;
    Ctx* c = reinterpret_cast<Ctx*>(h);
    PtState* s = c->pt.get();
    const size_t nchain = (size_t)s->T * s->R;
    hipError_t e = hipMemcpy(d_theta, s->d_theta, sizeof(double) * nchain * c->d, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_logpost, s->d_lp, sizeof(double) * nchain, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) return hip_fail(e, "carma_pt_bind_state");
    s->bind(d_theta, d_logpost);
    return CARMA_OK;
}

// Log-posteriors of chain states (starting values, carma_pt_set_chains without them) in launches of at most START_BATCH evaluations:
// which kernel a launch takes depends on its size (and, for the two-sided kernels on series of the SMALL class, on whether it leaves
// a CU to every workgroup), and a block of a sharded ladder or a rank's share of the replicas holds fewer chains than the
// single-process run -- its log-posteriors would come from another launch shape, a rounding apart, and the chains would no longer be
// the one-GPU run's bit for bit.  Below this size the choice does not depend on the count.
static int logdensity_of_chain_states(carma_ctx* h, const double* theta, size_t n, int d, double* out)
{
    constexpr size_t START_BATCH = 256;
    for (size_t i0 = 0; i0 < n; i0 += START_BATCH) {
        const size_t nb = std::min(START_BATCH, n - i0);
        const int rc = carma_logdensity_batch(h, theta + i0 * d, (int)nb, 0, out + i0);
        if (rc != CARMA_OK) return rc;
    }
    return CARMA_OK;
}

int carma_pt_set_chains(carma_ctx* h, const double* theta, const double* logpost)
{
    if (!h || !reinterpret_cast<Ctx*>(h)->pt || !theta) return CARMA_EINVAL;
    Ctx* c = reinterpret_cast<Ctx*>(h);
    PtState* s = c->pt.get();
    const size_t nchain = (size_t)s->T * s->R;
    std::vector<double> lp(nchain);
    if (logpost) {
        std::memcpy(lp.data(), logpost, sizeof(double) * nchain);
    } else {
        int rc = logdensity_of_chain_states(h, theta, nchain, c->d, lp.data());
        if (rc != CARMA_OK) return rc;
    }
    hipError_t e = pt_ens_set_chains(s, c->d, theta, lp.data());
    // a new set of chains starts a new history of boundary decisions: the two sides of a boundary compare folds of the
    // decisions since this point (carma_shard.hip), so one side re-created on its own must not inherit the old sum
    if (e == hipSuccess && s->d_checksum) e = hipMemset(s->d_checksum, 0, 4 * sizeof(unsigned long long));
    if (e != hipSuccess) return hip_fail(e, "carma_pt_set_chains");
    s->bnd_check = 0;
    s->started = true;
    return CARMA_OK;
}

int carma_pt_get_chains(carma_ctx* h, double* theta, double* logpost)
{
    if (!h || !reinterpret_cast<Ctx*>(h)->pt) return CARMA_EINVAL;
    Ctx* c = reinterpret_cast<Ctx*>(h);
    const hipError_t e = pt_ens_get_chains(c->pt.get(), c->d, theta, logpost);
    if (e != hipSuccess) return hip_fail(e, "carma_pt_get_chains");
    return CARMA_OK;
}

int carma_pt_start(carma_ctx* h, const double* init, int ninit)
{
    if (!h || !reinterpret_cast<Ctx*>(h)->pt) {
        set_error("carma_pt_start: call carma_pt_create first");
        return CARMA_EINVAL;
    }
    Ctx* c = reinterpret_cast<Ctx*>(h);
    PtState* s = c->pt.get();
    const int d = c->d;
    const size_t nchain = (size_t)s->T * s->R;
    std::vector<double> theta(nchain * d), lp(nchain, -std::numeric_limits<double>::infinity());
    std::vector<char> done(nchain, 0);
    // user-provided start is honoured only if its length is d and its posterior is finite
    // (src/samplers.cpp:75-93, src/carpack.cpp:479-490)
    if (init && ninit == d) {
        double l0 = 0;
        int rc = carma_logdensity_batch(h, init, 1, 0, &l0);
        if (rc != CARMA_OK) return rc;
        if (std::isfinite(l0)) {
            for (size_t k = 0; k < nchain; k++) {
                std::memcpy(&theta[k * d], init, sizeof(double) * d);
                lp[k] = l0;
                done[k] = 1;
            }
        }
    }
    // The draws of a chain are keyed by (seed, the chain's GLOBAL slot, attempt), not by the order in which a process
    // happens to visit its chains: a replica or a temperature gets the same starting value whichever rank holds it
    // (carma_pt_shard), so a sharded run starts -- and, the sampler's streams being keyed the same way, continues --
    // exactly as the single-process run does.
    const int rc = find_starts(
        nchain, d, theta.data(), lp.data(), done.data(),
        [&](size_t k, int round, double* out) {
            const uint64_t gslot = ((uint64_t)s->replica0 + k / (size_t)s->T) * (uint64_t)s->T_global + s->slot0 + k % (size_t)s->T;
            std::mt19937_64 rng = start_rng(s->seed, gslot, round);
            draw_start(c->t.data(), c->y.data(), c->n, c->pr, c->p, c->q, rng, out);
        },
        [&](const double* cand, const size_t*, size_t m, double* out) { return logdensity_of_chain_states(h, cand, m, d, out); });
    if (rc != CARMA_OK) return rc;
    for (size_t k = 0; k < nchain; k++) {
        if (!done[k]) {
            set_error("carma_pt_start: no finite starting value found for chain %zu", k);
            return CARMA_EINVAL;
        }
    }
    return carma_pt_set_chains(h, theta.data(), lp.data());
}

int carma_pt_iterate(carma_ctx* h, long niter, int do_exchange)
{
    if (!h || !reinterpret_cast<Ctx*>(h)->pt || niter < 0) return CARMA_EINVAL;
    Ctx* c = reinterpret_cast<Ctx*>(h);
    if (!c->pt->started) {
        set_error("carma_pt_iterate: chains have no starting values");
        return CARMA_EINVAL;
    }
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    return pt_launch_chunks(c, niter, do_exchange, 0, nullptr);
}

int carma_pt_sample(carma_ctx* h, int nsamples, int thin, double* samples, double* logposts)
{
    if (!h || !reinterpret_cast<Ctx*>(h)->pt || nsamples < 1 || thin < 1 || !samples || !logposts) {
        set_error("carma_pt_sample: bad argument");
        return CARMA_EINVAL;
    }
    Ctx* c = reinterpret_cast<Ctx*>(h);
    PtState* s = c->pt.get();
    if (!s->started) {
        set_error("carma_pt_sample: chains have no starting values");
        return CARMA_EINVAL;
    }
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    long capacity = 0;
    e = s->reserve_samples(c->d, nsamples, &capacity);
    if (e != hipSuccess) return hip_fail(e, "carma_pt_sample: sample buffers");
    long off = 0;
    int rc = pt_launch_chunks(c, (long)nsamples * thin, 1, thin, &off);
    if (rc == CARMA_OK) {
        e = pt_ens_fetch_samples(s, c->d, nsamples, samples, logposts);
        if (e != hipSuccess) rc = hip_fail(e, "D2H samples");
    }
    s->cap = capacity;
    return rc;
}

int carma_pt_stats(carma_ctx* h, double* accept_rate, double* swap_rate, int reset)
{
    if (!h || !reinterpret_cast<Ctx*>(h)->pt) return CARMA_EINVAL;
    const hipError_t e = pt_ens_stats(reinterpret_cast<Ctx*>(h)->pt.get(), accept_rate, swap_rate, reset);
    if (e != hipSuccess) return hip_fail(e, "carma_pt_stats");
    return CARMA_OK;
}

int carma_pt_kernel_in_use(const carma_ctx* h)
{
    if (!h || !reinterpret_cast<const Ctx*>(h)->pt) return CARMA_EINVAL;
    const PtState* s = reinterpret_cast<const Ctx*>(h)->pt.get();
    return s->use_row ? 1 : (s->use_lane ? 2 : 0);
}

int carma_pt_row_pipeline(void) { return pt_row_last_pipeline(); }

long carma_pt_iterations_done(const carma_ctx* h)
{
    if (!h || !reinterpret_cast<const Ctx*>(h)->pt) return CARMA_EINVAL;
    return (long)reinterpret_cast<const Ctx*>(h)->pt->iter;
}

int carma_pt_run(carma_ctx* h, int ntemps, int nreplicas, int sample_size, int burnin, int thin, const double* init,
                 int ninit, uint64_t seed, double* samples, double* logposts)
{
    int rc = carma_pt_create(h, ntemps, nreplicas, nullptr, burnin, seed);
    if (rc == CARMA_OK) rc = carma_pt_start(h, init, ninit);
    if (rc == CARMA_OK) rc = carma_pt_iterate(h, burnin, 1);                    // Sampler::Run burn-in (samplers.cpp:97)
    if (rc == CARMA_OK) rc = carma_pt_sample(h, sample_size, thin, samples, logposts);   // :101-108
    return rc;
}

}  // extern "C"
