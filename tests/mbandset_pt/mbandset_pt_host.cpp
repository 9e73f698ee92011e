// mbandset_pt_host.cpp -- carma_mband_set_pt_plan.h (the host-only decisions of the sampler over a set of multi-band objects)
// behind a C interface; test harness (tests/test_mbandset_pt_cpu.py).  It can run under the host sanitizers (g++
// -fsanitize=address,undefined with a main of its own); the tests build it plain.
#include <cstring>
#include <string>

#include "../../carma_pack_amd/csrc/carma_mband_set_pt_plan.h"

using namespace carma;

extern "C" {

long mbspt_run_waves(long RT) { return mbandset_pt_run_waves(RT); }
long mbspt_grid(long M, long RT) { return mbandset_pt_grid(M, RT); }

// wave b -> out3 = (run, first chain, live lanes)
void mbspt_wave(long b, long RT, long* out3)
{
    const MbandSetPtWave w = mbandset_pt_wave(b, RT);
    out3[0] = w.run;
    out3[1] = w.chain0;
    out3[2] = w.live;
}

// chain gi -> out2 = (wave, lane)
void mbspt_chain(long gi, long RT, long* out2)
{
    int lane = -1;
    mbandset_pt_chain(gi, RT, &out2[0], &lane);
    out2[1] = lane;
}

// -> 0 and msg = "" when the arguments are fine, 1 and the message otherwise
int mbspt_check_create(const int* run_obj, int M, int S, int ntemps, int nreplicas, int adapt_iters, int dx, int K, const int* n0,
                       const double* band_lo, const double* band_hi, char* msg, int len)
{
    const std::string s = mbandset_pt_check_create(run_obj, M, S, ntemps, nreplicas, adapt_iters, dx, K, n0, band_lo, band_hi);
    strncpy(msg, s.c_str(), (size_t)len - 1);
    msg[len - 1] = 0;
    return s.empty() ? 0 : 1;
}

long mbspt_chunk_iters(const int* run_obj, int M, const int* N) { return mbandset_pt_chunk_iters(run_obj, M, N); }
long mbspt_chunk_iters_single(int N) { return mband_pt_chunk_iters(N); }

}  // extern "C"
