// carma_pt_front.hip -- the entry points of the handle-based lane samplers over a PtFront (carma_pt_front.h): one chain per lane,
// an iteration as k_ram_propose / the front's K1 / k_ram_finish (launch_pt_lane_k1, carma_pt_lane.hip), a chunk in flight at a
// time.  Host code only: no kernel is defined here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "carma_pt_front.h"
#include "carma_pt_sched.h"

namespace carma {

// "<name>_<fn>", the name of an entry point as its messages carry it
static std::string entry(const PtFront& f, const char* fn)
{
    return std::string(f.name) + "_" + fn;
}

static int fail(const PtFront& f, const char* fn, hipError_t e)
{
    return hip_fail(e, entry(f, fn).c_str());
}

// the ensemble of f, or null with the error set: fn was called on a null handle, before create (need_start: or before the chains
// have starting values)
static PtEnsemble* front_state(const PtFront& f, const char* fn, bool need_start)
{
    if (!f.has_ctx) {
        set_error("%s_%s: null context", f.name, fn);
        return nullptr;
    }
    if (!f.s) {
        set_error("%s_%s: call %s_create first", f.name, fn, f.name);
        return nullptr;
    }
    if (need_start && !f.s->started) {
        set_error("%s_%s: chains have no starting values (%s_start / %s_set_chains)", f.name, fn, f.name, f.name);
        return nullptr;
    }
    return f.s;
}

// niter iterations, a chunk in flight at a time.  thin > 0: save the coldest chains every thin iterations from sample *save_offset
// on.  The stream is idle when this returns, whatever happened.
static int front_chunks(const PtFront& f, long niter, int do_exchange, int thin, long* save_offset)
{
    PtEnsemble* s = f.s;
    long left = niter;
    while (left > 0) {
        const long ch = pt_next_chunk(left, f.chunk0, thin);
        const PtLaunch L = pt_ens_launch(s, f.dim, f.q, f.n, ch, do_exchange, thin, save_offset ? *save_offset : 0);
        hipError_t e = launch_pt_lane_k1(f.p, L, s->d_scratch, f.k1, pt_ens_buffers(s), !s->factor_loaded, f.stream);
        if (e == hipSuccess) {
            s->factor_loaded = true;
            s->chol_stale = true;
        }
        const hipError_t es = hipStreamSynchronize(f.stream);
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) return hip_fail(e, (std::string(f.name) + ": sampler launch").c_str());
        pt_ens_advance(s, ch, thin, save_offset);
        left -= ch;
    }
    return CARMA_OK;
}

int pt_front_set_chains(const PtFront& f, const double* theta, const double* logpost)
{
    PtEnsemble* s = front_state(f, "set_chains", false);
    if (!s) return CARMA_EINVAL;
    if (!theta) {
        set_error("%s_set_chains: null theta", f.name);
        return CARMA_EINVAL;
    }
    const size_t nchain = s->nchain();
    std::vector<double> lp(nchain);
    if (logpost) {
        std::memcpy(lp.data(), logpost, sizeof(double) * nchain);
    } else {
        const int rc = f.eval(theta, nullptr, nchain, lp.data());   // one batch call over all chains
        if (rc != CARMA_OK) return rc;
    }
    hipError_t e = hipSetDevice(f.device);
    if (e == hipSuccess) e = pt_ens_set_chains(s, f.dim, theta, lp.data());
    if (e != hipSuccess) return fail(f, "set_chains", e);
    s->started = true;
    return CARMA_OK;
}

int pt_front_get_chains(const PtFront& f, double* theta, double* logpost)
{
    PtEnsemble* s = front_state(f, "get_chains", false);
    if (!s) return CARMA_EINVAL;
    hipError_t e = hipSetDevice(f.device);
    if (e == hipSuccess) e = pt_ens_get_chains(s, f.dim, theta, logpost);
    if (e != hipSuccess) return fail(f, "get_chains", e);
    return CARMA_OK;
}

int pt_front_start(const PtFront& f, const double* init)
{
    PtEnsemble* s = front_state(f, "start", false);
    if (!s) return CARMA_EINVAL;
    const size_t d = (size_t)f.dim, M = f.M, per_run = f.per_run, nchain = s->nchain();
    std::vector<double> theta(nchain * d), lp(nchain, -std::numeric_limits<double>::infinity());
    std::vector<char> done(nchain, 0);
    // a run's init row is honoured when its log-posterior is finite (src/samplers.cpp:75-93): it becomes every chain of that run;
    // all M rows in one call
    if (init) {
        std::vector<double> l0(M);
        std::vector<size_t> first(M);
        for (size_t j = 0; j < M; j++) first[j] = j * per_run;
        const int rc = f.eval(init, first.data(), M, l0.data());
        if (rc != CARMA_OK) return rc;
        for (size_t j = 0; j < M; j++) {
            if (!std::isfinite(l0[j])) continue;
            for (size_t k = j * per_run; k < (j + 1) * per_run; k++) {
                std::memcpy(&theta[k * d], init + j * d, sizeof(double) * d);
                lp[k] = l0[j];
                done[k] = 1;
            }
        }
    }
    // Drawn starts: chain k = ladder T + temperature of the ENSEMBLE keys its generator, so run j draws what a sampler of its own
    // sharded to replica0 = j R draws; the candidates still pending of ALL runs are evaluated in one call per round.
    const int rc = find_starts(nchain, f.dim, theta.data(), lp.data(), done.data(), f.draw, f.eval);
    if (rc != CARMA_OK) return rc;
    for (size_t k = 0; k < nchain; k++)
        if (!done[k]) {
            set_error("%s_start: no finite starting value found for %s", f.name, f.which(k).c_str());
            return CARMA_EINVAL;
        }
    return pt_front_set_chains(f, theta.data(), lp.data());
}

// get / set of the proposal factors; a failure drains the stream, on which the copies of the caller's array were enqueued
static int front_factor(const PtFront& f, const char* fn, double* get, const double* set)
{
    PtEnsemble* s = front_state(f, fn, false);
    if (!s) return CARMA_EINVAL;
    if (!get && !set) {
        set_error("%s_%s: null chol", f.name, fn);
        return CARMA_EINVAL;
    }
    hipError_t e = hipSetDevice(f.device);
    if (e == hipSuccess) e = get ? pt_ens_get_factor(s, f.dim, f.stream, get) : pt_ens_set_factor(s, f.dim, f.stream, set);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(f.stream);
        return fail(f, fn, e);
    }
    return CARMA_OK;
}

int pt_front_get_factor(const PtFront& f, double* chol) { return front_factor(f, "get_factor", chol, nullptr); }
int pt_front_set_factor(const PtFront& f, const double* chol) { return front_factor(f, "set_factor", nullptr, chol); }

int pt_front_iterate(const PtFront& f, long niter, int do_exchange)
{
    if (!front_state(f, "iterate", true)) return CARMA_EINVAL;
    if (niter < 0) {
        set_error("%s_iterate: niter < 0", f.name);
        return CARMA_EINVAL;
    }
    const hipError_t e = hipSetDevice(f.device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    return front_chunks(f, niter, do_exchange, 0, nullptr);
}

int pt_front_sample(const PtFront& f, int nsamples, int thin, double* samples, double* logposts)
{
    PtEnsemble* s = front_state(f, "sample", true);
    if (!s) return CARMA_EINVAL;
    if (nsamples < 1 || thin < 1 || !samples || !logposts) {
        set_error("%s_sample: bad argument (nsamples >= 1, thin >= 1, non-null outputs)", f.name);
        return CARMA_EINVAL;
    }
    hipError_t e = hipSetDevice(f.device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    long capacity = 0;
    e = s->reserve_samples(f.dim, nsamples, &capacity);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s_sample: no device memory for the sample buffer: %zu bytes asked for (%ld ladders x %d samples x %d)", f.name,
                  sizeof(double) * (size_t)s->R * nsamples * (f.dim + 1), (long)s->R, nsamples, f.dim);
        return CARMA_ENOMEM;
    }
    long off = 0;
    int rc = front_chunks(f, (long)nsamples * thin, 1, thin, &off);
    if (rc == CARMA_OK) {
        e = pt_ens_fetch_samples(s, f.dim, nsamples, samples, logposts);
        if (e != hipSuccess) rc = hip_fail(e, (entry(f, "sample") + ": D2H").c_str());
    }
    s->cap = capacity;
    return rc;
}

int pt_front_stats(const PtFront& f, double* accept_rate, double* swap_rate, int reset)
{
    PtEnsemble* s = front_state(f, "stats", false);
    if (!s) return CARMA_EINVAL;
    hipError_t e = hipSetDevice(f.device);
    if (e == hipSuccess) e = pt_ens_stats(s, accept_rate, swap_rate, reset);
    if (e != hipSuccess) return fail(f, "stats", e);
    return CARMA_OK;
}

long pt_front_iterations_done(const PtFront& f)
{
    return f.s ? (long)f.s->iter : (long)CARMA_EINVAL;
}

int pt_front_logdensity(const PtFront& f, const double* theta, double* out)
{
    PtEnsemble* s = front_state(f, "logdensity", false);
    if (!s) return CARMA_EINVAL;
    if (!theta || !out) {
        set_error("%s_logdensity: null theta or out", f.name);
        return CARMA_EINVAL;
    }
    const size_t nchain = s->nchain(), d = (size_t)f.dim, GUARD = 64;
    // [nc][dim] proposals, [nc] results, then GUARD words nobody may write: a kernel whose idle lanes stored would show here
    std::vector<double> res(nchain + GUARD, 0.0);
    const double mark = -12345.678;
    std::fill(res.begin() + nchain, res.end(), mark);
    hipError_t e = hipSetDevice(f.device);
    if (e == hipSuccess) e = f.guard->need(sizeof(double) * (nchain * d + nchain + GUARD));
    double *d_th = f.guard->as<double>(), *d_ll = d_th + nchain * d;
    if (e == hipSuccess) e = hipMemcpyAsync(d_th, theta, sizeof(double) * nchain * d, hipMemcpyHostToDevice, f.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_ll, res.data(), sizeof(double) * res.size(), hipMemcpyHostToDevice, f.stream);
    if (e == hipSuccess) e = f.k1(d_th, (long)nchain, d_ll, f.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(res.data(), d_ll, sizeof(double) * res.size(), hipMemcpyDeviceToHost, f.stream);
    const hipError_t es = hipStreamSynchronize(f.stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(f, "logdensity", e);
    for (size_t k = nchain; k < res.size(); k++)
        if (res[k] != mark) {
            set_error("%s_logdensity: the kernel wrote past its %zu results", f.name, nchain);
            return CARMA_EHIP;
        }
    std::memcpy(out, res.data(), sizeof(double) * nchain);
    return CARMA_OK;
}

int pt_front_run(const PtFront& f, const double* init, int burnin, int sample_size, int thin, double* samples, double* logposts)
{
    int rc = pt_front_start(f, init);
    if (rc == CARMA_OK) rc = pt_front_iterate(f, burnin, 1);                             // Sampler::Run burn-in (samplers.cpp:97)
    if (rc == CARMA_OK) rc = pt_front_sample(f, sample_size, thin, samples, logposts);   // :101-108
    return rc;
}

}  // namespace carma
