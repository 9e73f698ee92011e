// carma_host.h -- host-side state behind the C ABI (carma_capi.hip, carma_pt_host.hip): device allocation (carma_devbuf.h), the
// model rows the kernels read (carma_model_pack.h), the single-series context Ctx, and the state the two parallel-tempering
// samplers share (PtEnsemble and its pt_ens_* functions; the host-only decisions of the samplers -- ladder, initial factor,
// chunking, starting values -- are in carma_pt_sched.h)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "carma_devbuf.h"
#include "carma_launch.h"
#include "carma_model_pack.h"
#include "carma_types.h"

namespace carma {

// What both parallel-tempering samplers hold: an ensemble of R ladders of T chains (chain = ladder * T + temperature) with its
// buffers.  carma_pt_* (PtState below): the R replicas of one series; carma_mpt_* (MptState, carma_mseries.h): the ladders of
// all runs of a call.  The pt_ens_* functions (carma_pt_host.hip) work on this part alone.
struct PtEnsemble {
    int T = 0, R = 0;                  // temperatures of a ladder, ladders (what PtLaunch::T and ::R receive)
    int maxiter = 0;
    uint64_t seed = 0;
    unsigned long long iter = 0, stat_iters = 0;
    bool started = false;
    std::vector<double> temps;
    double *d_temps = nullptr, *d_theta = nullptr, *d_lp = nullptr, *d_chol = nullptr;
    unsigned *d_nacc = nullptr, *d_nswap = nullptr;
    double *d_samples = nullptr, *d_slp = nullptr;
    long cap = 0;                      // samples per ladder d_samples / d_slp hold; during a sampling call: that call's stride
    // lane sampler (carma_pt_lane.hip): one chain per lane, an iteration as propose kernel + batched log-density + finish kernel;
    // the factors live in the chain-minor scratch between calls
    double* d_scratch = nullptr;       // chain-minor working state (current value, R^T z, packed factor, proposals, ...)
    bool factor_loaded = false;        // the scratch holds the current factors (else: take them from d_chol at the next launch)
    bool chol_stale = false;           // d_chol is behind the scratch (pt_ens_sync_factor brings it up to date)
    bool ext_state = false;            // d_theta / d_lp belong to the caller (carma_pt_bind_state)
    size_t nchain() const { return (size_t)T * R; }
};

// Parallel-tempering sampler state of one context (carma_pt_host.hip, carma_shard.hip): the ensemble, and which kernel runs it
struct PtState : PtEnsemble {
    unsigned T_global = 0, slot0 = 0, replica0 = 0;
    // row-variant kernel (k_pt_row): ladders spread over wpl workgroups, swap through global staging
    bool use_row = false;
    int wpl = 0;
    unsigned long long* d_stage = nullptr;      // tagged staging words of the swap step (PtRowSync::stage)
    unsigned long long epoch = 0;               // launches so far (PtRowSync::epoch)
    unsigned* d_abort = nullptr;
    double* d_backup = nullptr;         // chain state before the chunk in flight (theta, logpost, chol): abort recovery
    bool use_lane = false;              // large ensembles: the lane sampler (d_scratch)
    // ladder sharded across ranks (carma_shard.hip): boundary staging and statistics
    double *d_send = nullptr, *d_recv = nullptr;       // [R][d+1] each
    unsigned* d_bnd_swaps = nullptr;                   // [1] accepted boundary swaps (this block's side)
    unsigned long long bnd_proposed = 0;
    unsigned long long* d_checksum = nullptr;          // [4] folds of the boundary decisions: lower / upper side, the peers' reports
    int bnd_check = 0;                                 // result of the last self-check: 1 agreed, -1 differed, 0 none yet
};

struct Ctx {
    int device = 0;
    int p = 0, q = 0, d = 0, n = 0;
    std::vector<double> t, y, yerr;   // after sort/dedup
    Prior pr{};
    int sflags = 0;                   // SERIES_* of the series under the prior (series_flags, carma_shape_plan.h)
    int series_flags() const { return sflags; }
    double* d_series = nullptr;       // records {dt, y, yerr^2, t}[n + 16 pads], then yerr^2[n + 16], y[n + 16] (carma_types.h)
    double* d_theta = nullptr;        // staging for the host-pointer entry points
    double* d_out = nullptr;
    double* h_stage = nullptr;        // pinned host staging: [cap * d] parameter vectors followed by [cap] results
    int cap = 0;
    hipStream_t stream = nullptr;
    PtState* pt = nullptr;
    int ensure_staging(int B);
};

void set_error(const char* fmt, ...);
// series preparation shared by carma_ctx_create and carma_mctx_create (carma_capi.hip)
void sort_dedup(std::vector<double>& t, std::vector<double>& y, std::vector<double>& e);
std::vector<double> pack_series(const std::vector<double>& t, const std::vector<double>& y, const std::vector<double>& e);
void set_prior_bounds(Prior& pr, const double* t, long n, double max_stdev);
int hip_fail(hipError_t e, const char* what);
int select_device(int device);
void pt_state_free(Ctx* c);
// Enqueue `niter` iterations of the sampler kernel on `st` (no synchronisation).  thin > 0: save the coldest chain
// every `thin` iterations starting at sample index *save_offset (advanced).
int pt_enqueue(Ctx* c, long niter, int do_exchange, int thin, long* save_offset, hipStream_t st);
// after the stream has been synchronised: did a cross-workgroup rendezvous of the row kernel time out?
int pt_check_abort(Ctx* c, bool* aborted);

// ---- the ensemble (PtEnsemble) of either sampler; d: parameter dimension.  The hipError_t ones leave the failure to the entry point.
// R ladders of T chains with their buffers: allocated, temps[T] and the factors chol[R * T][d * d] uploaded, counters zeroed
hipError_t pt_ens_create(PtEnsemble* s, int T, int R, int d, const std::vector<double>& temps, const double* chol);
void pt_ens_release(PtEnsemble* s);   // every device buffer of the ensemble (not the caller's: ext_state)
// arguments of a launch of ch iterations from the current one: the whole ensemble is the whole ladder (slot0 = 0, T_global = T,
// replica0 = 0); n: (longest) series length
PtLaunch pt_ens_launch(const PtEnsemble* s, int d, int q, int n, long ch, int do_exchange, int thin, long save_offset);
void pt_ens_advance(PtEnsemble* s, long ch, int thin, long* save_offset);   // ... and the books after it has been enqueued
hipError_t pt_ens_set_chains(PtEnsemble* s, int d, const double* theta, const double* lp);
hipError_t pt_ens_get_chains(const PtEnsemble* s, int d, double* theta, double* lp);   // either may be null
// Room for nsamples per ladder, which become the stride of the launches that follow (PtLaunch::sample_cap); *capacity: what the
// buffers hold, for the caller to put back into s->cap when the call ends.  fetch: those samples, [R][nsamples][d] and [R][nsamples]
hipError_t pt_ens_reserve_samples(PtEnsemble* s, int d, int nsamples, long* capacity);
hipError_t pt_ens_fetch_samples(const PtEnsemble* s, int d, int nsamples, double* samples, double* logposts);
// rates per chain since the last reset (entry i of swap_rate = swaps between temperature i and i - 1); either may be null
hipError_t pt_ens_stats(PtEnsemble* s, double* accept_rate, double* swap_rate, int reset);
// The lane sampler keeps the proposal factors in its scratch between calls.  sync: bring the chain-major array d_chol up to date
// before it is read (enqueued on st; nothing to do after the other kernels); written: d_chol was written, the next launch reloads.
// get / set: [R][T][d * d] to and from the host, after what is in flight on st.
hipError_t pt_ens_sync_factor(PtEnsemble* s, int d, hipStream_t st);
void pt_ens_factor_written(PtEnsemble* s);
hipError_t pt_ens_get_factor(PtEnsemble* s, int d, hipStream_t st, double* chol);
hipError_t pt_ens_set_factor(PtEnsemble* s, int d, hipStream_t st, const double* chol);

}  // namespace carma
