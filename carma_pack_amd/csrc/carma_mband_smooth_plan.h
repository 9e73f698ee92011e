// carma_mband_smooth_plan.h -- the host-only decisions of carma_bands_smooth (carma_mband_smooth.hip): the requested times as the
// lanes walk them, the strides of the scratch records, the rows of a chunk and the argument checks.  Plain C++, no HIP: compiled
// stand-alone by tests/mband_smooth/plan_main.cpp.
#ifndef CARMA_MBAND_SMOOTH_PLAN_H
#define CARMA_MBAND_SMOOTH_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <limits>
#include <numeric>
#include <string>
#include <vector>

#include "carma_smooth_plan.h"

namespace carma {

// The requested times of one output band, sorted once for every lane: a lane sees the time tout at tout - lag_bo, the same shift
// for all of them, so this order is every lane's.  Equal times keep the caller's order (stable).
//   perm[M]        sorted time r = the caller's tout[perm[r]]
//   rec[M + 1][4]  {tout - t0, perm[r] (the slot the result goes to), 0, 0}, then the sentinel {+inf, 0, 1, 0}; t0: the origin
//                  mband_pack took from the data times
struct MbandSmoothTimes {
    std::vector<int> perm;
    std::vector<double> rec;
};

inline MbandSmoothTimes mband_smooth_times(const double* tout, int M, double t0)
{
    MbandSmoothTimes s;
    s.perm.resize(M);
    std::iota(s.perm.begin(), s.perm.end(), 0);
    std::stable_sort(s.perm.begin(), s.perm.end(), [&](int a, int b) { return tout[a] < tout[b]; });
    s.rec.reserve(4 * ((size_t)M + 1));
    for (int r = 0; r < M; r++) {
        s.rec.push_back(tout[s.perm[r]] - t0);
        s.rec.push_back((double)s.perm[r]);
        s.rec.push_back(0.0);
        s.rec.push_back(0.0);
    }
    s.rec.push_back(std::numeric_limits<double>::infinity());
    s.rec.push_back(0.0);
    s.rec.push_back(1.0);
    s.rec.push_back(0.0);
    return s;
}

// Scratch of the two passes, [wave][point][field][64] doubles: a point's record is k[p], cr[p], sr of every pair [p / 2] and
// {pm, f, s, innov or slot, a_b} (carma_mband_smooth.h), every field one row of the wave's 64 lanes.
struct MbandSmoothStrides {
    int fields = 0;           // doubles of a point's record
    long fs = 0, ps = 0;      // from field to field, from point to point (doubles)
    size_t ws = 0;            // from wave to wave
};

constexpr int mband_smooth_nfields(int p) { return 2 * p + p / 2 + 5; }

inline MbandSmoothStrides mband_smooth_strides(int p, int ng)
{
    MbandSmoothStrides s;
    s.fields = mband_smooth_nfields(p);
    s.fs = 64;
    s.ps = 64L * s.fields;
    s.ws = (size_t)ng * (size_t)s.ps;
    return s;
}

// bytes of scratch a row (one parameter vector) takes
inline size_t mband_smooth_row_bytes(int p, int ng) { return (size_t)ng * mband_smooth_nfields(p) * sizeof(double); }

struct MbandSmoothChunks {
    long rows = 0;            // rows per chunk (the last chunk may hold fewer)
    long waves = 0;           // waves (= workgroups) of a full chunk
    long chunks = 0;          // launches of each pass
    size_t bytes = 0;         // scratch of a full chunk
};

// forced: rows per chunk asked for ("MBAND_SMOOTH_CHUNK_ROWS"; <= 0: automatic, as many whole waves as the cap holds, one at least)
inline MbandSmoothChunks mband_smooth_chunks(int p, int ng, long B, long forced, size_t cap = SMOOTH_SCRATCH_CAP)
{
    MbandSmoothChunks c;
    const size_t wb = std::max<size_t>(1, 64 * mband_smooth_row_bytes(p, ng));
    long rows = forced > 0 ? forced : (long)std::max<size_t>(1, cap / wb) * 64;
    rows = std::max(1L, std::min(rows, std::max(1L, B)));
    c.rows = rows;
    c.waves = (rows + 63) / 64;
    c.chunks = (std::max(1L, B) + rows - 1) / rows;
    c.bytes = (size_t)c.waves * wb;
    return c;
}

// What carma_bands_smooth refuses, as a message ("" = fine).  K, N: bands and data of the handle (ignored
// without one).
inline std::string mband_smooth_check(bool have_handle, int K, long N, const double* theta, int B, int band, const double* tout, int M,
                                      const double* mean, const double* var, const double* bmean, const double* bvar)
{
    char buf[256];
    if (!have_handle) return "null handle";
    if (B < 1 || M < 1) {
        snprintf(buf, sizeof(buf), "need B >= 1 and M >= 1 (got B = %d, M = %d)", B, M);
        return buf;
    }
    if (!theta || !tout) return "need non-null theta and tout";
    if (band < 0 || band >= K) {
        snprintf(buf, sizeof(buf), "band %d is outside [0, %d)", band, K);
        return buf;
    }
    if ((mean == nullptr) != (var == nullptr) || (bmean == nullptr) != (bvar == nullptr) || (!mean && !bmean))
        return "mean and var, band_mean and band_var come in pairs, and one pair at least is needed";
    for (int i = 0; i < M; i++)
        if (!std::isfinite(tout[i])) {
            snprintf(buf, sizeof(buf), "tout[%d] is not finite", i);
            return buf;
        }
    if (N + (long)M > 0x7fffffffL) return "more data and requested times than an int can count";
    return "";
}

}  // namespace carma

#endif
