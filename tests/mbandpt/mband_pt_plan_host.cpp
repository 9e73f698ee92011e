// mband_pt_plan_host.cpp -- carma_mband_pt_plan.h (the host-only decisions of the bands sampler) and ram_kernels_plan of
// carma_shape_plan.h behind a C interface; test harness (tests/mband_pt_build.py).  It can run under the host sanitizers
// (g++ -fsanitize=address,undefined with a main of its own); the tests build it plain.
// bands: t / y concatenated, off = [K + 1].
#include <cstring>
#include <string>
#include <vector>

#include "../../carma_pack_amd/csrc/carma_mband_pt_plan.h"
#include "../../carma_pack_amd/csrc/carma_shape_plan.h"

using namespace carma;

static std::vector<BandView> views(const double* t, const double* y, const long* off, int K)
{
    std::vector<BandView> v((size_t)K);
    for (int b = 0; b < K; b++) v[b] = BandView{t + off[b], y + off[b], (int)(off[b + 1] - off[b])};
    return v;
}

extern "C" {

// -> 0 and msg = "" when the arguments are fine, 1 and the message otherwise
int mbpt_check_create(int ntemps, int nreplicas, int adapt_iters, int dx, int K, int n0, const double* band_lo, const double* band_hi,
                      char* msg, int len)
{
    const std::string s = mband_pt_check_create(ntemps, nreplicas, adapt_iters, dx, K, n0, band_lo, band_hi);
    strncpy(msg, s.c_str(), (size_t)len - 1);
    msg[len - 1] = 0;
    return s.empty() ? 0 : 1;
}

void mbpt_initial_factor(const double* t, const double* y, const long* off, int K, int d, double* R0)
{
    const std::vector<BandView> b = views(t, y, off, K);
    mband_pt_initial_factor(b.data(), K, d, R0);
}

// prior = max_stdev, max_freq, min_freq, measerr_dof
void mbpt_draw_start(const double* t, const double* y, const long* off, int K, const double* prior, int p, int q, const double* lagbox,
                     unsigned long long seed, unsigned long long chain, int round, double* thx)
{
    const std::vector<BandView> b = views(t, y, off, K);
    Prior pr{prior[0], prior[1], prior[2], prior[3]};
    mband_pt_draw_start(b.data(), K, pr, p, q, lagbox, seed, chain, round, thx);
}

void mbpt_default_box(const double* t, const double* y, const long* off, int K, double* lo, double* hi)
{
    const std::vector<BandView> b = views(t, y, off, K);
    mband_pt_default_box(b.data(), K, lo, hi);
}

int mbpt_in_box(const double* thx, int d, int K, const double* lo, const double* hi) { return mband_pt_in_box(thx, d, K, lo, hi) ? 1 : 0; }

long mbpt_chunk_iters(int N) { return mband_pt_chunk_iters(N); }

// RamKernels as an int: 0 none, 1 fused, 2 split, 3 wide; have_min = 0: the tune entry unset
int mbpt_ram_kernels_plan(int d, int have_min, long wide_min)
{
    ShapeSwitches sw;
    if (have_min) sw.pt_ram_wide_min = wide_min;
    return (int)ram_kernels_plan(d, sw);
}

}  // extern "C"
