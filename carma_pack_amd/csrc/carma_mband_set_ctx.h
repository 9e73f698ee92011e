// carma_mband_set_ctx.h -- the context behind a carma_bandset handle, shared by the files that serve it (carma_mband_set.hip:
// log-density and optimiser; carma_mband_set_smooth.hip: smoother; carma_mband_set_pt.hip: sampler).  Host C++ only.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "carma_devbuf.h"
#include "carma_mband_set_plan.h"
#include "carma_pt_state.h"

namespace carma {

// Sampler state of a set context (carma_bandset_pt_*): M runs of R replicas (ladders) of T chains, run j on object run_obj[j]:
// ONE ensemble of M R ladders, run j its ladders j R ... j R + R - 1
struct BSptState : PtEnsemble {
    int M = 0, reps = 0;              // runs, replicas per run (R of the ensemble = M reps)
    std::vector<int> run_obj;         // [M]
    DevBuf<int> d_run_obj;            // ... on the device, uploaded once at create
    bool has_box = false;
    std::vector<double> box;          // [M][2][K - 1][2]: per run lo then hi of (log a_b, mu_b), when has_box
    DevBuf<double> d_box;             // ... on the device
    int nmax = 0;                     // data of the longest object among the runs
    long chunk0 = 1;                  // iterations per chunk (mbandset_pt_chunk_iters)
    DevMem k_res;                     // per-call buffer of carma_bandset_pt_logdensity, grown on demand
};

// A set of multi-band objects: the prepared objects side by side (MbandSet, carma_mband_set_plan.h; its records are dropped once
// they are on the device) and the set's device state
struct BSctx {
    int device = 0;
    int p = 0, q = 0, d = 0, K = 0, dx = 0, S = 0;
    MbandSet m;
    std::vector<char> plain;          // [S] zeros: the launch plan's cadence classes, of which a set has one
    DevMem d_rec, d_off, d_boff, d_N, d_lagbox, d_pr;
    WaveBatch wb;                     // per-call buffers and launch plan of carma_bandset_logdensity_batch (carma_devbuf.h)
    hipStream_t stream = nullptr;
    std::unique_ptr<BSptState> bspt;  // the sampler, after carma_bandset_pt_create
};

}  // namespace carma
