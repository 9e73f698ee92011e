// carma_mband_ctx.h -- the multi-band context behind a carma_bands handle, shared by the files that serve it (carma_mband.hip:
// log-density and optimiser; carma_mband_smooth.hip: smoother; carma_mband_pt.hip: sampler).  Host C++ only.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "carma_devbuf.h"
#include "carma_mband_plan.h"
#include "carma_pt_state.h"
#include "carma_types.h"

namespace carma {

// Sampler state of a multi-band context (carma_bands_pt_*): one run of R replicas (ladders) of T chains on the extended vector
struct BptState : PtEnsemble {
    bool has_box = false;
    std::vector<double> box;          // [2][K - 1][2]: lo then hi of (log a_b, mu_b), when has_box
    DevBuf<double> d_box;             // ... on the device
};

// Multi-band context: one prepared object (MbandObject, carma_mband_plan.h: n, N, boff, lagbox, pr, t0 and the bands' sorted
// times and values, the sampler's starting values; its records are dropped once they are on the device) and its device state
struct Bctx {
    int device = 0;
    int p = 0, q = 0, d = 0, K = 0, dx = 0;
    MbandObject o;
    DevMem d_rec, d_boff, d_lagbox;   // the records of all bands in one buffer, a sentinel behind each band
    DevMem d_theta, d_out;            // per-call buffers of the host-pointer entry point, grown on demand
    hipStream_t stream = nullptr;
    std::unique_ptr<BptState> bpt;    // the sampler, after carma_bands_pt_create
};

}  // namespace carma
