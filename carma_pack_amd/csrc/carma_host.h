// carma_host.h -- host-side state behind the C ABI (carma_capi.hip, carma_pt_host.hip): the owners of device and pinned memory
// (carma_devbuf.h), the model rows the kernels read (carma_model_pack.h), the single-series context Ctx, and the pt_ens_* functions
// on the state the two parallel-tempering samplers share (PtEnsemble, carma_pt_state.h, which also holds every buffer request of
// the samplers; their host-only decisions -- ladder, initial factor, chunking, starting values -- are in carma_pt_sched.h).
// A handle owns all its memory: deleting it, on its device, releases everything.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

#include "carma_devbuf.h"
#include "carma_launch.h"
#include "carma_model_pack.h"
#include "carma_prep.h"
#include "carma_pt_state.h"
#include "carma_types.h"

namespace carma {

struct Ctx {
    int device = 0;
    int p = 0, q = 0, d = 0, n = 0;
    std::vector<double> t, y, yerr;   // after sort/dedup
    Prior pr{};
    int sflags = 0;                   // SERIES_* of the series under the prior (series_flags, carma_shape_plan.h)
    int series_flags() const { return sflags; }
    DevBuf<double> d_series;          // records {dt, y, yerr^2, t}[n + 16 pads], then yerr^2[n + 16], y[n + 16] (carma_types.h)
    const double4* rec() const { return reinterpret_cast<const double4*>(d_series.get()); }
    DevBuf<double> d_theta, d_out;    // staging for the host-pointer entry points
    PinnedBuf<double> h_stage;        // pinned host staging: [cap * d] parameter vectors followed by [cap] results
    int cap = 0;
    hipStream_t stream = nullptr;
    std::unique_ptr<PtState> pt;
    int ensure_staging(int B);
};

void set_error(const char* fmt, ...);
// series preparation shared by carma_ctx_create and carma_mctx_create: sort_dedup, set_prior_bounds and the default max_stdev
// are host-only text in carma_prep.h; the packer is in carma_capi.hip
std::vector<double> pack_series(const std::vector<double>& t, const std::vector<double>& y, const std::vector<double>& e);
int hip_fail(hipError_t e, const char* what);
int select_device(int device);
// Enqueue `niter` iterations of the sampler kernel on `st` (no synchronisation).  thin > 0: save the coldest chain
// every `thin` iterations starting at sample index *save_offset (advanced).
int pt_enqueue(Ctx* c, long niter, int do_exchange, int thin, long* save_offset, hipStream_t st);
// after the stream has been synchronised: did a cross-workgroup rendezvous of the row kernel time out?
int pt_check_abort(Ctx* c, bool* aborted);

// ---- the ensemble (PtEnsemble) of either sampler; d: parameter dimension.  The hipError_t ones leave the failure to the entry point.
// R ladders of T chains with their buffers: allocated, temps[T] and the factors chol[R * T][d * d] uploaded, counters zeroed
hipError_t pt_ens_create(PtEnsemble* s, int T, int R, int d, const std::vector<double>& temps, const double* chol);
// the eight pointers of the ensemble the sampler launchers take (carma_launch.h)
inline PtBuffers pt_ens_buffers(const PtEnsemble* s)
{
    return {s->d_temps, s->d_theta, s->d_lp, s->d_chol, s->d_nacc, s->d_nswap, s->d_samples, s->d_slp};
}
// arguments of a launch of ch iterations from the current one: the whole ensemble is the whole ladder (slot0 = 0, T_global = T,
// replica0 = 0); n: (longest) series length
PtLaunch pt_ens_launch(const PtEnsemble* s, int d, int q, int n, long ch, int do_exchange, int thin, long save_offset);
void pt_ens_advance(PtEnsemble* s, long ch, int thin, long* save_offset);   // ... and the books after it has been enqueued
hipError_t pt_ens_set_chains(PtEnsemble* s, int d, const double* theta, const double* lp);
hipError_t pt_ens_get_chains(const PtEnsemble* s, int d, double* theta, double* lp);   // either may be null
// the samples of a call that reserved nsamples per ladder (PtEnsemble::reserve_samples), [R][nsamples][d] and [R][nsamples]
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
