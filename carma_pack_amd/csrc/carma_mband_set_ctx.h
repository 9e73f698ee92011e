// carma_mband_set_ctx.h -- the context behind a carma_bandset handle, shared by the files that serve it (carma_mband_set.hip:
// log-density and optimiser; carma_mband_set_smooth.hip: smoother).  Host C++ only.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "carma_devbuf.h"
#include "carma_mband_set_plan.h"

namespace carma {

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
};

}  // namespace carma
