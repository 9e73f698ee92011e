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
#include "carma_pt_front.h"

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

// The sampler of h as the shared front drives it (carma_pt_front.h).  A row is evaluated on the object, and inside the box, of its
// chain's run; chain k draws from ITS object with the generator its slot in the ensemble keys, so run j draws what
// carma_bands_pt_start draws for ladders j R ... on a handle of its object.
static PtFront bspt_front(carma_bandset* h)
{
    PtFront f;
    f.name = "carma_bandset_pt";
    if (!h) return f;
    BSctx* c = reinterpret_cast<BSctx*>(h);
    BSptState* s = c->bspt.get();
    f.has_ctx = true;
    f.device = c->device;
    f.stream = c->stream;
    f.p = c->p;
    f.q = c->q;
    f.dim = c->dx;
    f.s = s;
    if (!s) return f;
    const size_t per_run = (size_t)s->reps * s->T;
    f.M = (size_t)s->M;
    f.per_run = per_run;
    f.n = s->nmax;
    f.chunk0 = s->chunk0;
    f.guard = &s->k_res;
    f.k1 = [c, s](const double* thn, long nc, double* ll, hipStream_t st) { return launch_logdens_mband_chains_ms(c, s, thn, nc, ll, st); };
    f.eval = [h, s, per_run](const double* rows, const size_t* chain, size_t m, double* out) {
        std::vector<int> run(m);
        for (size_t i = 0; i < m; i++) run[i] = (int)((chain ? chain[i] : i) / per_run);
        return bspt_logdens_host(h, s, rows, run.data(), m, out);
    };
    // (the runs' band views are made at the first draw: only start draws)
    f.draw = [c, s, per_run, views = std::vector<std::vector<BandView>>()](size_t k, int round, double* out) mutable {
        if (views.empty())
            for (int j = 0; j < s->M; j++) views.push_back(band_views(c, s->run_obj[j]));
        const size_t j = k / per_run;
        const int sj = s->run_obj[j];
        mband_pt_draw_start(views[j].data(), c->K, c->m.pr[sj], c->p, c->q, c->m.lagbox.data() + (size_t)sj * 2 * (c->K - 1), s->seed,
                            (uint64_t)k, round, out);
    };
    f.which = [s, per_run](size_t k) {
        char buf[96];
        snprintf(buf, sizeof(buf), "chain %zu of run %zu (object %d)", k % per_run, k / per_run, s->run_obj[k / per_run]);
        return std::string(buf);
    };
    return f;
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
    return pt_front_set_chains(bspt_front(h), theta, logpost);
}

int carma_bandset_pt_get_chains(carma_bandset* h, double* theta, double* logpost)
{
    return pt_front_get_chains(bspt_front(h), theta, logpost);
}

int carma_bandset_pt_start(carma_bandset* h, const double* init) { return pt_front_start(bspt_front(h), init); }

int carma_bandset_pt_get_factor(carma_bandset* h, double* chol) { return pt_front_get_factor(bspt_front(h), chol); }

int carma_bandset_pt_set_factor(carma_bandset* h, const double* chol) { return pt_front_set_factor(bspt_front(h), chol); }

int carma_bandset_pt_iterate(carma_bandset* h, long niter, int do_exchange) { return pt_front_iterate(bspt_front(h), niter, do_exchange); }

int carma_bandset_pt_sample(carma_bandset* h, int nsamples, int thin, double* samples, double* logposts)
{
    return pt_front_sample(bspt_front(h), nsamples, thin, samples, logposts);
}

int carma_bandset_pt_stats(carma_bandset* h, double* accept_rate, double* swap_rate, int reset)
{
    return pt_front_stats(bspt_front(h), accept_rate, swap_rate, reset);
}

long carma_bandset_pt_iterations_done(const carma_bandset* h)
{
    return pt_front_iterations_done(bspt_front(const_cast<carma_bandset*>(h)));
}

int carma_bandset_pt_logdensity(carma_bandset* h, const double* theta, double* out)
{
    return pt_front_logdensity(bspt_front(h), theta, out);
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
    const int rc = carma_bandset_pt_create(h, run_obj, M, ntemps, nreplicas, nullptr, burnin, seed, band_lo, band_hi);
    return rc == CARMA_OK ? pt_front_run(bspt_front(h), init, burnin, sample_size, thin, samples, logposts) : rc;
}

}  // extern "C"
