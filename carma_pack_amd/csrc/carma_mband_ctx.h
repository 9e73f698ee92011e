// carma_mband_ctx.h -- the multi-band context behind a carma_bands handle, shared by the files that serve it (carma_mband.hip:
// log-density and optimiser; carma_mband_smooth.hip: smoother).  Host C++ only.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "carma_devbuf.h"
#include "carma_types.h"

namespace carma {

// Multi-band context: the records of all bands in one buffer, a sentinel behind each band
struct Bctx {
    int device = 0;
    int p = 0, q = 0, d = 0, K = 0, dx = 0, N = 0;
    std::vector<int> n, boff;         // [K] data per band, [K + 1] first record of a band (mband_pack)
    std::vector<double> lagbox;       // [K - 1][2]
    double t0 = 0.0;                  // the time origin mband_pack subtracted: the earliest time of all bands
    Prior pr{};
    DevMem d_rec, d_boff, d_lagbox;
    DevMem d_theta, d_out;            // per-call buffers of the host-pointer entry point, grown on demand
    hipStream_t stream = nullptr;
};

}  // namespace carma
