// carma_mband_pt.hip -- the SAMPLER of a multi-band fit (carma_bands_pt_*): the large-ensemble
// sampler of carma_pt_lane.hip -- one chain per lane, an iteration as propose / K1 / finish -- on the extended vector of a
// carma_bands handle, [dx = 3 + p + q + 3 (K - 1)]: the CARMA part, then (lag_b, log a_b, mu_b) per further band.  K1 is
// k_logdens_carma_mband_chains: the merged Kalman filter of carma_mband.h, one chain per lane, plus the sampler's band box
// (carma_mband_pt_plan.h).  The bookkeeping is launch_pt_lane_k1's: the templated kernels up to dx = 16, the wide ones beyond
// (ram_kernels_plan).  One run of R replicas x T temperatures; host-only decisions in carma_mband_pt_plan.h.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "grp_device.h"
#include "carma_core.h"
#include "carma_lane.h"
#include "carma_mband.h"
#include "carma_host.h"
#include "carma_mband_ctx.h"
#include "carma_mband_pt_plan.h"
#include "carma_pt_front.h"

namespace carma {

static_assert(MBAND_PT_DMAX == RAM_DMAX_WIDE, "carma_mband_pt_plan.h and carma_shape_plan.h disagree on the widest chain");

// K1 of the bands sampler: ONE CHAIN PER LANE, chain gi = 64 blockIdx.x + threadIdx.x; thn = [nc][dx] chain-major (the proposals
// the bookkeeping kernels write), ll = [nc].  The body is logdensity_mband_lane with the prior, as k_logdens_carma_mband calls it:
// inside the box a chain gets that kernel's bits.  box = [2][K - 1][2], lo then hi of (log a_b, mu_b), or null: a chain with a
// band term outside (or NaN) gets -inf.  Lanes past nc shadow the wave's first chain and write nothing.
template <int P>
__global__ __launch_bounds__(64) void k_logdens_carma_mband_chains(const double* __restrict__ thn, int dx, int q, int K, int N,
                                                                  const double4* __restrict__ rec, const int* __restrict__ boff,
                                                                  const double* __restrict__ lagbox, const double* __restrict__ box,
                                                                  Prior pr, long nc, double* __restrict__ ll)
{
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];   // all LDS is dynamic (mband_lds_bytes)
    const int lane = threadIdx.x;
    MbandWork wk;
    const double* s_tab = mband_lds_carve(s_dyn, K, K, lane, boff, 0, wk);
    long gi = (long)blockIdx.x * 64 + lane;
    const bool live = gi < nc;
    if (!live) gi = (long)blockIdx.x * 64;
    const double* thx = thn + gi * dx;
    double v = logdensity_mband_lane<P>(thx, q, K, N, rec, lagbox, pr, 0, s_tab, wk);
    if (box) {
        const int d = dx - 3 * (K - 1), nb = 2 * (K - 1);
        bool in = true;
        for (int i = 0; i < nb; i++) {
            const double x = thx[d + 3 * (i >> 1) + 1 + (i & 1)];
            in = in && x >= box[i] && x <= box[nb + i];
        }
        if (!in) v = -1.0 / 0.0;
    }
    if (live) ll[gi] = v;
}

static hipError_t launch_logdens_mband_chains(const Bctx* c, const BptState* s, const double* thn, long nc, double* ll, hipStream_t st)
{
    (void)hipGetLastError();   // HIP's last-error is sticky: drop anything left by earlier calls
    if (nc <= 0) return hipSuccess;
    const dim3 grid((unsigned)((nc + 63) / 64)), block(64);
    const size_t lds = mband_lds_bytes(c->K);
    const double* box = s->has_box ? s->d_box.get() : nullptr;
    auto go = [&](auto P) {
        hipLaunchKernelGGL((k_logdens_carma_mband_chains<decltype(P)::value>), grid, block, lds, st, thn, c->dx, c->q, c->K, c->o.N,
                           c->d_rec.as<const double4>(), c->d_boff.as<const int>(), c->d_lagbox.as<const double>(), box, c->o.pr, nc, ll);
        return hipGetLastError();
    };
    if (c->p == 1) return go(std::integral_constant<int, 1>{});   // (for_order starts at 2: CAR(1) is the generic body at P = 1 here)
    return for_order(c->p, hipErrorInvalidValue, go);
}

static std::vector<BandView> band_views(const Bctx* c)
{
    std::vector<BandView> v((size_t)c->K);
    for (int b = 0; b < c->K; b++) v[b] = BandView{c->o.ts[b].data(), c->o.ys[b].data(), c->o.n[b]};
    return v;
}

// the log-density a chain of the sampler has at thx [m][dx]: the library's, with the prior, and -inf outside the band box
static int bpt_logdens_host(carma_bands* h, const BptState* s, const double* thx, size_t m, double* out)
{
    Bctx* c = reinterpret_cast<Bctx*>(h);
    const int rc = carma_bands_logdensity_batch(h, thx, (int)m, 0, out);
    if (rc != CARMA_OK || !s->has_box) return rc;
    const size_t nb = 2 * (size_t)(c->K - 1);
    for (size_t i = 0; i < m; i++)
        if (!mband_pt_in_box(thx + i * c->dx, c->d, c->K, s->box.data(), s->box.data() + nb)) out[i] = -std::numeric_limits<double>::infinity();
    return CARMA_OK;
}

// The sampler of h as the shared front drives it (carma_pt_front.h): one run, so every chain is of run 0
static PtFront bpt_front(carma_bands* h)
{
    PtFront f;
    f.name = "carma_bands_pt";
    if (!h) return f;
    Bctx* c = reinterpret_cast<Bctx*>(h);
    BptState* s = c->bpt.get();
    f.has_ctx = true;
    f.device = c->device;
    f.stream = c->stream;
    f.p = c->p;
    f.q = c->q;
    f.dim = c->dx;
    f.s = s;
    f.guard = &c->d_theta;
    if (!s) return f;
    f.per_run = s->nchain();
    f.n = c->o.N;
    f.chunk0 = mband_pt_chunk_iters(c->o.N);
    f.k1 = [c, s](const double* thn, long nc, double* ll, hipStream_t st) { return launch_logdens_mband_chains(c, s, thn, nc, ll, st); };
    f.eval = [h, s](const double* rows, const size_t*, size_t m, double* out) { return bpt_logdens_host(h, s, rows, m, out); };
    f.draw = [c, s, bands = band_views(c)](size_t k, int round, double* out) {
        mband_pt_draw_start(bands.data(), c->K, c->o.pr, c->p, c->q, c->o.lagbox.data(), s->seed, (uint64_t)k, round, out);
    };
    f.which = [s](size_t k) {
        char buf[96];
        snprintf(buf, sizeof(buf), "chain %zu (temperature %zu of replica %zu)", k, k % (size_t)s->T, k / (size_t)s->T);
        return std::string(buf);
    };
    return f;
}

}  // namespace carma

using namespace carma;

extern "C" {

int carma_bands_pt_default_box(const carma_bands* h, double* band_lo, double* band_hi)
{
    if (!h || !band_lo || !band_hi) {
        set_error("carma_bands_pt_default_box: null context or output");
        return CARMA_EINVAL;
    }
    const Bctx* c = reinterpret_cast<const Bctx*>(h);
    const std::vector<BandView> bands = band_views(c);
    mband_pt_default_box(bands.data(), c->K, band_lo, band_hi);
    return CARMA_OK;
}

int carma_bands_pt_create(carma_bands* h, int ntemps, int nreplicas, const double* temperatures, int adapt_iters, uint64_t seed,
                          const double* band_lo, const double* band_hi)
{
    if (!h) {
        set_error("carma_bands_pt_create: null context");
        return CARMA_EINVAL;
    }
    Bctx* c = reinterpret_cast<Bctx*>(h);
    const std::string bad = mband_pt_check_create(ntemps, nreplicas, adapt_iters, c->dx, c->K, c->o.n[0], band_lo, band_hi);
    if (!bad.empty()) {
        set_error("carma_bands_pt_create: %s", bad.c_str());
        return CARMA_EINVAL;
    }
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    c->bpt.reset(new BptState());         // (the state of an earlier call goes, with every buffer it holds)
    BptState* s = c->bpt.get();
    s->maxiter = adapt_iters;
    s->seed = seed;
    std::vector<double> temps;
    default_ladder(ntemps, temperatures, temps);
    const int dx = c->dx;
    const size_t nchain = (size_t)nreplicas * ntemps, nb = 2 * (size_t)(c->K - 1);
    const std::vector<BandView> bands = band_views(c);
    std::vector<double> R0((size_t)dx * dx), chol(nchain * dx * dx);
    mband_pt_initial_factor(bands.data(), c->K, c->d, R0.data());
    for (size_t k = 0; k < nchain; k++) std::memcpy(&chol[k * dx * dx], R0.data(), sizeof(double) * dx * dx);
    s->has_box = band_lo != nullptr && nb > 0;
    if (s->has_box) {
        s->box.assign(band_lo, band_lo + nb);
        s->box.insert(s->box.end(), band_hi, band_hi + nb);
    }
    e = pt_ens_create(s, ntemps, nreplicas, dx, temps, chol.data());
    if (e == hipSuccess) e = s->d_scratch.alloc(pt_lane_scratch_doubles(dx, (long)nchain));
    if (e == hipSuccess && s->has_box) e = s->d_box.alloc(2 * nb);
    if (e == hipSuccess && s->has_box) e = hipMemcpy(s->d_box, s->box.data(), sizeof(double) * 2 * nb, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        c->bpt.reset();
        return hip_fail(e, "carma_bands_pt_create");
    }
    return CARMA_OK;
}

int carma_bands_pt_set_chains(carma_bands* h, const double* theta, const double* logpost)
{
    return pt_front_set_chains(bpt_front(h), theta, logpost);
}

int carma_bands_pt_get_chains(carma_bands* h, double* theta, double* logpost) { return pt_front_get_chains(bpt_front(h), theta, logpost); }

int carma_bands_pt_start(carma_bands* h, const double* init) { return pt_front_start(bpt_front(h), init); }

int carma_bands_pt_get_factor(carma_bands* h, double* chol) { return pt_front_get_factor(bpt_front(h), chol); }

int carma_bands_pt_set_factor(carma_bands* h, const double* chol) { return pt_front_set_factor(bpt_front(h), chol); }

int carma_bands_pt_iterate(carma_bands* h, long niter, int do_exchange) { return pt_front_iterate(bpt_front(h), niter, do_exchange); }

int carma_bands_pt_sample(carma_bands* h, int nsamples, int thin, double* samples, double* logposts)
{
    return pt_front_sample(bpt_front(h), nsamples, thin, samples, logposts);
}

int carma_bands_pt_stats(carma_bands* h, double* accept_rate, double* swap_rate, int reset)
{
    return pt_front_stats(bpt_front(h), accept_rate, swap_rate, reset);
}

long carma_bands_pt_iterations_done(const carma_bands* h) { return pt_front_iterations_done(bpt_front(const_cast<carma_bands*>(h))); }

int carma_bands_pt_logdensity(carma_bands* h, const double* theta, double* out) { return pt_front_logdensity(bpt_front(h), theta, out); }

int carma_bands_pt_kernel_name(const carma_bands* h, char* buf, int len)
{
    if (!h || !buf || len < 1) return CARMA_EINVAL;
    const Bctx* c = reinterpret_cast<const Bctx*>(h);
    return snprintf(buf, len, "k_logdens_carma_mband_chains<%d>", c->p) > 0 ? CARMA_OK : CARMA_EINVAL;
}

int carma_bands_pt_run(carma_bands* h, int ntemps, int nreplicas, int sample_size, int burnin, int thin, const double* init,
                       uint64_t seed, const double* band_lo, const double* band_hi, double* samples, double* logposts)
{
    const int rc = carma_bands_pt_create(h, ntemps, nreplicas, nullptr, burnin, seed, band_lo, band_hi);
    return rc == CARMA_OK ? pt_front_run(bpt_front(h), init, burnin, sample_size, thin, samples, logposts) : rc;
}

}  // extern "C"
