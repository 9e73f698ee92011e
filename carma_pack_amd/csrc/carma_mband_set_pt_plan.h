// carma_mband_set_pt_plan.h -- what the sampler over a SET of multi-band objects (carma_bandset_pt_*, carma_mband_set_pt.hip)
// decides on the host: the wave map of its log-density kernel, the argument checks of its create call and the chunk size.  Host
// C++ only, no HIP runtime: tests/mbandset_pt/mbandset_pt_host.cpp puts it behind a C interface for the CPU tests.
//
// A RUN is one sampler (R replicas x T temperatures) on one object of the set; a call's M runs are the ladders j R ... j R + R - 1
// of ONE ensemble of M R ladders (carma_mpt.hip), run j owning chains [j RT, (j + 1) RT), RT = R T.  What a run decides from its
// object -- the initial factor, the default box, the starting draw, the box test -- are the functions of carma_mband_pt_plan.h,
// called with that object's BandViews; nothing of them is repeated here.
//
// THE WAVE MAP.  A wave works on ONE object (the band offsets in LDS, the trip count, the lag boxes and the prior stay
// wave-uniform, as in k_logdens_carma_mband_ms), so a wave never spans two runs: with W = ceil(RT / 64) waves a run, wave b
// serves run b / W, its chains 64 (b % W) ... of that run; the lanes past the run's last chain are pads.  Everything derives
// from the wave's index and RT: no table is built per call.
#ifndef CARMA_MBAND_SET_PT_PLAN_H
#define CARMA_MBAND_SET_PT_PLAN_H

#include <algorithm>
#include <cstdio>
#include <string>

#include "carma_mband_pt_plan.h"

namespace carma {

constexpr int MBANDSET_PT_LANES = 64;

// waves a run of RT chains takes, and the grid of M runs
inline long mbandset_pt_run_waves(long RT) { return (RT + MBANDSET_PT_LANES - 1) / MBANDSET_PT_LANES; }
inline long mbandset_pt_grid(long M, long RT) { return M * mbandset_pt_run_waves(RT); }

// wave b of the grid: its run, its first chain (of the ensemble) and how many of its lanes are live (>= 1: lane 0 always is)
struct MbandSetPtWave {
    long run, chain0;
    int live;
};
inline MbandSetPtWave mbandset_pt_wave(long b, long RT)
{
    const long W = mbandset_pt_run_waves(RT), j = b / W, w = b % W;
    return MbandSetPtWave{j, j * RT + MBANDSET_PT_LANES * w, (int)std::min<long>(MBANDSET_PT_LANES, RT - MBANDSET_PT_LANES * w)};
}

// chain gi of the ensemble: the wave that serves it and its lane there
inline void mbandset_pt_chain(long gi, long RT, long* wave, int* lane)
{
    const long j = gi / RT, k = gi % RT;
    *wave = j * mbandset_pt_run_waves(RT) + k / MBANDSET_PT_LANES;
    *lane = (int)(k % MBANDSET_PT_LANES);
}

// What carma_bandset_pt_create refuses, as a message ("" = fine): M >= 1, every run's object in [0, S), M R T chains within what a
// launch indexes, then mband_pt_check_create of every run with ITS object's n[0] (n0 = [S]) and ITS box (band_lo / band_hi =
// [M][K - 1][2], both or neither), the run and its object named.
inline std::string mbandset_pt_check_create(const int* run_obj, int M, int S, int ntemps, int nreplicas, int adapt_iters, int dx, int K,
                                            const int* n0, const double* band_lo, const double* band_hi)
{
    char buf[512];
    if (!run_obj) return "need a non-null list of runs";
    if (M < 1) {
        snprintf(buf, sizeof(buf), "need at least one run (got M = %d)", M);
        return buf;
    }
    for (int j = 0; j < M; j++)
        if (run_obj[j] < 0 || run_obj[j] >= S) {
            snprintf(buf, sizeof(buf), "run %d (object %d): object index out of range (nobjects = %d)", j, run_obj[j], S);
            return buf;
        }
    if (nreplicas >= 1 && ntemps >= 1 && ntemps <= 64) {
        const long long nc = (long long)M * nreplicas * ntemps;
        if (nc > MBAND_PT_CHAINS_MAX) {
            const int j = (int)(MBAND_PT_CHAINS_MAX / ((long long)nreplicas * ntemps));   // the first run whose chains do not fit
            snprintf(buf, sizeof(buf), "run %d (object %d): %d runs x %d replicas x %d temperatures = %lld chains, more than one launch can index (%lld)",
                     j, run_obj[j], M, nreplicas, ntemps, nc, MBAND_PT_CHAINS_MAX);
            return buf;
        }
    }
    if ((band_lo == nullptr) != (band_hi == nullptr)) return "band_lo and band_hi come together (both null: no box)";
    const size_t nb = 2 * (size_t)(K - 1);
    for (int j = 0; j < M; j++) {
        const std::string bad = mband_pt_check_create(ntemps, nreplicas, adapt_iters, dx, K, n0[run_obj[j]],
                                                      band_lo ? band_lo + (size_t)j * nb : nullptr,
                                                      band_hi ? band_hi + (size_t)j * nb : nullptr);
        if (!bad.empty()) {
            snprintf(buf, sizeof(buf), "run %d (object %d): %s", j, run_obj[j], bad.c_str());
            return buf;
        }
    }
    return "";
}

// Iterations per chunk: an iteration's K1 runs as long as its longest object (N = [S], the data of all bands per object), so
// the chunk is mband_pt_chunk_iters of the largest N among the objects of the call's runs
inline long mbandset_pt_chunk_iters(const int* run_obj, int M, const int* N)
{
    int nmax = 1;
    for (int j = 0; j < M; j++) nmax = std::max(nmax, N[run_obj[j]]);
    return mband_pt_chunk_iters(nmax);
}

}  // namespace carma

#endif
