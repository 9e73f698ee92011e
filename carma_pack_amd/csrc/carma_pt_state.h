// carma_pt_state.h -- the state of the parallel-tempering samplers and the part of them that only requests, regrows and releases
// device buffers: which buffers a state holds, how many elements each, in which order they are asked for, and what is left after a
// request failed.  Every buffer has an owner (carma_devbuf.h), so deleting a state releases all of it; the copies, memsets and
// launches are in carma_pt_host.hip, carma_shard.hip and carma_pt_front.hip.  Host C++ without the HIP runtime:
// tests/hostmem/hostmem_main.cpp runs these methods over an allocator of its own.
#pragma once
#include <cstdint>
#include <vector>

#include "carma_devbuf.h"

namespace carma {

// What every parallel-tempering sampler holds: an ensemble of R ladders of T chains (chain = ladder * T + temperature) with its
// buffers.  carma_pt_* (PtState below): the R replicas of one series; the handle-based lane samplers behind carma_pt_front.h --
// carma_mpt_* (MptState), carma_bands_pt_* (BptState, carma_mband_ctx.h), carma_bandset_pt_* (BSptState, carma_mband_set_ctx.h):
// the ladders of all runs of a call.  The pt_ens_* functions (carma_host.h, carma_pt_host.hip) work on this part alone.
struct PtEnsemble {
    int T = 0, R = 0;                  // temperatures of a ladder, ladders (what PtLaunch::T and ::R receive)
    int maxiter = 0;
    uint64_t seed = 0;
    unsigned long long iter = 0, stat_iters = 0;
    bool started = false;
    std::vector<double> temps;
    DevBuf<double> d_temps, d_chol;
    DevBuf<unsigned> d_nacc, d_nswap;
    // The chain state the kernels read and write: views.  They show the library's own two buffers until the caller binds memory of
    // its own (carma_pt_bind_state), which releases those; the caller's memory has no owner here and is never released.
    double *d_theta = nullptr, *d_lp = nullptr;
    DevBuf<double> own_theta, own_lp, d_samples, d_slp;
    long cap = 0;                      // samples per ladder d_samples / d_slp hold; during a sampling call: that call's stride
    // lane sampler (carma_pt_lane.hip): one chain per lane, an iteration as propose kernel + batched log-density + finish kernel;
    // the factors live in the chain-minor scratch between calls
    DevBuf<double> d_scratch;          // chain-minor working state (current value, R^T z, packed factor, proposals, ...)
    bool factor_loaded = false;        // the scratch holds the current factors (else: take them from d_chol at the next launch)
    bool chol_stale = false;           // d_chol is behind the scratch (pt_ens_sync_factor brings it up to date)
    size_t nchain() const { return (size_t)T * R; }

    // the buffers of R_ ladders of T_ chains of dimension d
    hipError_t reserve(int T_, int R_, int d)
    {
        T = T_;
        R = R_;
        hipError_t e = d_temps.alloc(T);
        if (e == hipSuccess) e = own_theta.alloc(nchain() * d);
        if (e == hipSuccess) e = own_lp.alloc(nchain());
        if (e == hipSuccess) e = d_chol.alloc(nchain() * d * d);
        if (e == hipSuccess) e = d_nacc.alloc(nchain());
        if (e == hipSuccess) e = d_nswap.alloc(nchain());
        d_theta = own_theta;
        d_lp = own_lp;
        return e;
    }
    // the chain state lives in the caller's memory from now on (the caller has copied it there)
    void bind(double* theta, double* lp)
    {
        own_theta.release();
        own_lp.release();
        d_theta = theta;
        d_lp = lp;
    }
    // Room for nsamples per ladder, which become the stride of the launches that follow (PtLaunch::sample_cap); *capacity: what the
    // buffers hold, for the caller to put back into cap when the call ends.  Both buffers or neither: after a failure cap is 0.
    hipError_t reserve_samples(int d, int nsamples, long* capacity)
    {
        if (cap < nsamples) {
            d_samples.release();
            d_slp.release();
            cap = 0;
            hipError_t e = d_samples.alloc((size_t)R * nsamples * d);
            if (e == hipSuccess) e = d_slp.alloc((size_t)R * nsamples);
            if (e != hipSuccess) {
                d_samples.release();
                return e;
            }
            cap = nsamples;
        }
        *capacity = cap;
        cap = nsamples;   // stride of this call's output
        return hipSuccess;
    }
};

// Parallel-tempering sampler state of one context (carma_pt_host.hip, carma_shard.hip): the ensemble, and which kernel runs it
struct PtState : PtEnsemble {
    unsigned T_global = 0, slot0 = 0, replica0 = 0;
    // row-variant kernel (k_pt_row): ladders spread over wpl workgroups, swap through global staging
    bool use_row = false;
    int wpl = 0;
    DevBuf<unsigned long long> d_stage;         // tagged staging words of the swap step (PtRowSync::stage)
    unsigned long long epoch = 0;               // launches so far (PtRowSync::epoch)
    DevBuf<unsigned> d_abort;
    DevBuf<double> d_backup;            // chain state before the chunk in flight (theta, logpost, chol): abort recovery
    bool use_lane = false;              // large ensembles: the lane sampler (d_scratch)
    // ladder sharded across ranks (carma_shard.hip): boundary staging and statistics
    DevBuf<double> d_send, d_recv;                     // [R][d+1] (+ the boundary temperature) each
    DevBuf<unsigned> d_bnd_swaps;                      // [1] accepted boundary swaps (this block's side)
    unsigned long long bnd_proposed = 0;
    DevBuf<unsigned long long> d_checksum;             // [4] folds of the boundary decisions: lower / upper side, the peers' reports
    int bnd_check = 0;                                 // result of the last self-check: 1 agreed, -1 differed, 0 none yet

    // row kernel: tagged staging (two buffers x two copies of (theta[d], log-posterior) per chain), abort flag, backup
    hipError_t reserve_row(int d)
    {
        hipError_t e = d_stage.alloc(4 * nchain() * (d + 1));
        if (e == hipSuccess) e = d_abort.alloc(1);
        if (e == hipSuccess) e = d_backup.alloc(nchain() * (d + 1 + (size_t)d * d));
        return e;
    }
    // The four boundary buffers of a sharded ladder, nbuf doubles to a side: all four or none, so that a call after a failed one
    // asks again (d_send alone says whether they are there).
    hipError_t reserve_boundary(size_t nbuf)
    {
        hipError_t e = d_send.alloc(nbuf);
        if (e == hipSuccess) e = d_recv.alloc(nbuf);
        if (e == hipSuccess) e = d_bnd_swaps.alloc(1);
        if (e == hipSuccess) e = d_checksum.alloc(4);
        if (e != hipSuccess) release_boundary();
        return e;
    }
    void release_boundary()
    {
        d_send.release();
        d_recv.release();
        d_bnd_swaps.release();
        d_checksum.release();
    }
};

// Sampler state of a multi-series context (carma_mpt_*): M runs of `reps` ladders of T chains = one ensemble of R = M reps ladders
struct MptState : PtEnsemble {
    int M = 0, reps = 0;              // runs, replicas per run
    std::vector<int> series;          // [M] series of run j
    int nmax = 0;                     // the longest series of the call
    long chunk0 = 1;                  // iterations per chunk (mpt_chunk_iters, carma_mseries_plan.h)
    bool any_plain = false, any_rep = false;   // the call holds irregular / regular-cadence series
    DevBuf<int> d_lser;               // [R] series of every ladder, uploaded once
    DevBuf<char> d_rep;               // [S] SERIES_REPEATED_DT of every series
};

}  // namespace carma
