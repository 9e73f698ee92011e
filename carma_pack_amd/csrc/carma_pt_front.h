// carma_pt_front.h -- the one front of the handle-based lane samplers (carma_mpt_*, carma_bands_pt_*, carma_bandset_pt_*): what
// an entry point does once it knows which K1 evaluates the proposals, where a chain's starting draw comes from and how a row is
// evaluated on the host.  Each of the three files fills a PtFront from its handle in one function and its extern "C" functions
// call the pt_front_* functions below; create, default_box, kernel_name, the K1 and the host evaluator stay with the file.
// carma_pt_* (carma_pt_host.hip) is another engine and does not come through here.
#pragma once
#include <functional>
#include <string>

#include "carma_host.h"

namespace carma {

// A handle's lane sampler.  has_ctx = false (a null handle): only `name` is meaningful.
struct PtFront {
    const char* name = "";            // C prefix, for messages: "carma_mpt", "carma_bands_pt", "carma_bandset_pt"
    bool has_ctx = false;
    int device = 0;
    hipStream_t stream = nullptr;
    int p = 0, q = 0, dim = 0;        // dim: length of a chain's vector (d, or dx of the band samplers)
    PtEnsemble* s = nullptr;          // null before create
    size_t M = 1, per_run = 0;        // runs, chains of a run: chain k belongs to run k / per_run
    int n = 0;                        // what PtLaunch::n receives: the (longest) series length
    long chunk0 = 1;                  // iterations per chunk
    DevMem* guard = nullptr;          // per-call buffer of the guarded log-density, grown on demand
    PtLaneK1 k1;
    // out[i] = log-posterior of rows[i][dim], a candidate of chain chain[i] (null: of chain i), i < m; CARMA_OK or the error
    std::function<int(const double* rows, const size_t* chain, size_t m, double* out)> eval;
    std::function<void(size_t k, int round, double* out)> draw;   // starting draw of chain k of the ensemble in this round
    std::function<std::string(size_t k)> which;                   // "chain ... of run ..." for the no-finite-start message
};

// fn: the entry point without the prefix ("set_chains"); messages read "<name>_<fn>: ..."
int pt_front_set_chains(const PtFront& f, const double* theta, const double* logpost);
int pt_front_get_chains(const PtFront& f, double* theta, double* logpost);
// init [M][dim] or null: a run's row becomes every chain of that run when its log-posterior is finite; the rest is drawn
int pt_front_start(const PtFront& f, const double* init);
int pt_front_get_factor(const PtFront& f, double* chol);
int pt_front_set_factor(const PtFront& f, const double* chol);
// The stream is idle when these return, whatever happened.
int pt_front_iterate(const PtFront& f, long niter, int do_exchange);
int pt_front_sample(const PtFront& f, int nsamples, int thin, double* samples, double* logposts);
int pt_front_stats(const PtFront& f, double* accept_rate, double* swap_rate, int reset);
long pt_front_iterations_done(const PtFront& f);
// K1 over the whole ensemble at theta [nchain][dim], with guard words behind the results that no lane may write
int pt_front_logdensity(const PtFront& f, const double* theta, double* out);
// what follows create in *_pt_run: start, burn-in, sampling
int pt_front_run(const PtFront& f, const double* init, int burnin, int sample_size, int thin, double* samples, double* logposts);

}  // namespace carma
