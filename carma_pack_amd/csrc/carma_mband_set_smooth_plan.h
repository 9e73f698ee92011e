// carma_mband_set_smooth_plan.h -- the host-only decisions of carma_bandset_smooth (carma_mband_set_smooth.hip): the argument
// checks, the jobs, the waves with their tables and the chunks that share the scratch.  Pure functions of plain arrays, in the
// manner of msmooth_plan (carma_mseries_plan.h) and carma_mband_smooth_plan.h.  Plain C++, no HIP: compiled stand-alone by
// tests/mbandset_smooth/plan_main.cpp.
//
// Row i of a call is (theta[i], object[i], band[i], the times tout[toff[i] ... toff[i + 1])).  The rows are stably sorted by
// (object, band, number of times, the times one by one); a run of equal keys is a JOB: one object, one output band, one list of
// requested times -- what a wave's walk is uniform in.  The rows of a job fill waves of 64 in the caller's order, the last wave
// of a job padded with -1 (pads only trail, lane 0 of a wave is live).  The waves come with the largest ng = N_s + M first, ties
// in job order.
//   wave_job [W]                              job of wave w
//   job_obj, job_band, job_M [J], job_req [J] object, output band and number of times of job j, its first request record
//   req                                       the jobs' request records, mband_smooth_times(times, M, t0[object]), concatenated
//   row_idx [64 W]                            lane l of wave w works on the caller's row row_idx[64 w + l], -1: a pad lane
//   wave_sc [W]                               first double of wave w's records [point][field][64] inside its chunk's scratch
//   out_off [B]                               toff[i] - toff[0]: where row i's results go
// Chunks of consecutive waves [chunk0[c], chunk0[c + 1]) reuse one scratch buffer of sc_max doubles: a chunk ends before the wave
// that would take it past the cap or past `forced` waves ("MBANDSET_SMOOTH_CHUNK_WAVES"; <= 0: no such limit), and holds one wave
// at least.  A row's result does not depend on the chunking.
#ifndef CARMA_MBAND_SET_SMOOTH_PLAN_H
#define CARMA_MBAND_SET_SMOOTH_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#include "carma_mband_smooth_plan.h"

namespace carma {

// What carma_bandset_smooth refuses, as a message ("" = fine).  S, K, nobj = [S]: objects, bands and data per object of the
// handle (not read without one).  The times are read last: a row whose N_s + M_i an int cannot count is refused before them.
inline std::string mbandset_smooth_check(bool have_handle, int S, int K, const int* nobj, const double* theta, const int* object,
                                         const int* band, int B, const double* tout, const long* toff, const double* mean,
                                         const double* var)
{
    char buf[256];
    if (!have_handle) return "null handle";
    if (B < 1) {
        snprintf(buf, sizeof(buf), "need B >= 1 (got B = %d)", B);
        return buf;
    }
    if (!theta || !object || !band || !tout || !toff || !mean || !var) return "need non-null theta, object, band, tout, toff, mean and var";
    if (toff[0] < 0) {
        snprintf(buf, sizeof(buf), "toff[0] = %ld is negative", toff[0]);
        return buf;
    }
    for (int i = 0; i < B; i++) {
        if (object[i] < 0 || object[i] >= S) {
            snprintf(buf, sizeof(buf), "object[%d] = %d out of range (nobjects = %d)", i, object[i], S);
            return buf;
        }
        if (band[i] < 0 || band[i] >= K) {
            snprintf(buf, sizeof(buf), "band[%d] = %d is outside [0, %d)", i, band[i], K);
            return buf;
        }
        if (toff[i + 1] - toff[i] < 1) {
            snprintf(buf, sizeof(buf), "row %d has no times: toff must grow by at least 1 a row (toff[%d] = %ld, toff[%d] = %ld)", i, i,
                     toff[i], i + 1, toff[i + 1]);
            return buf;
        }
        if ((long)nobj[object[i]] + (toff[i + 1] - toff[i]) > 0x7fffffffL) {
            snprintf(buf, sizeof(buf), "row %d: more data and requested times than an int can count", i);
            return buf;
        }
    }
    for (int i = 0; i < B; i++)
        for (long k = toff[i]; k < toff[i + 1]; k++)
            if (!std::isfinite(tout[k])) {
                snprintf(buf, sizeof(buf), "time %ld of row %d is not finite", k - toff[i], i);
                return buf;
            }
    return "";
}

struct MbandSetSmoothPlan {
    long W = 0, J = 0;
    std::vector<int> wave_job, job_obj, job_band, job_M, row_idx;
    std::vector<long> job_req, wave_sc, out_off, chunk0;
    std::vector<double> req;
    size_t sc_max = 0;                // doubles of the largest chunk's scratch
};

// Arguments that mbandset_smooth_check has passed; nobj, t0 = [S]: data and time origin of every object (MbandSet::N, ::t0)
inline MbandSetSmoothPlan mbandset_smooth_plan(int p, const int* object, const int* band, int B, const double* tout, const long* toff,
                                               const int* nobj, const double* t0, long forced, size_t cap = SMOOTH_SCRATCH_CAP)
{
    MbandSetSmoothPlan pl;
    auto len = [&](int i) { return toff[i + 1] - toff[i]; };
    auto cmp = [&](int a, int b) {                            // <0, 0, >0
        if (object[a] != object[b]) return object[a] < object[b] ? -1 : 1;
        if (band[a] != band[b]) return band[a] < band[b] ? -1 : 1;
        if (len(a) != len(b)) return len(a) < len(b) ? -1 : 1;
        for (long k = 0; k < len(a); k++) {
            const double x = tout[toff[a] + k], y = tout[toff[b] + k];
            if (x != y) return x < y ? -1 : 1;
        }
        return 0;
    };
    pl.out_off.resize((size_t)B);
    for (int i = 0; i < B; i++) pl.out_off[i] = toff[i] - toff[0];
    std::vector<int> ord((size_t)B);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return cmp(a, b) < 0; });
    // the jobs, and the waves in job order: wave v is rows ord[first[v] ... first[v] + count[v])
    std::vector<int> wjob, count;
    std::vector<size_t> first;
    for (size_t k = 0; k < ord.size();) {
        size_t k1 = k + 1;
        while (k1 < ord.size() && cmp(ord[k], ord[k1]) == 0) k1++;
        const int i0 = ord[k], s = object[i0], M = (int)len(i0), job = (int)pl.job_obj.size();
        const MbandSmoothTimes tm = mband_smooth_times(tout + toff[i0], M, t0[s]);
        pl.job_obj.push_back(s);
        pl.job_band.push_back(band[i0]);
        pl.job_M.push_back(M);
        pl.job_req.push_back((long)(pl.req.size() / 4));
        pl.req.insert(pl.req.end(), tm.rec.begin(), tm.rec.end());
        for (size_t a = k; a < k1; a += 64) {
            wjob.push_back(job);
            first.push_back(a);
            count.push_back((int)std::min<size_t>(64, k1 - a));
        }
        k = k1;
    }
    pl.J = (long)pl.job_obj.size();
    const long W = pl.W = (long)wjob.size();
    auto ng = [&](int job) { return (long)nobj[pl.job_obj[job]] + pl.job_M[job]; };
    std::vector<long> wo((size_t)W);
    std::iota(wo.begin(), wo.end(), 0L);
    std::stable_sort(wo.begin(), wo.end(), [&](long a, long b) { return ng(wjob[a]) > ng(wjob[b]); });
    pl.wave_job.resize((size_t)W);
    pl.row_idx.assign((size_t)W * 64, -1);
    for (long w = 0; w < W; w++) {
        const long v = wo[w];
        pl.wave_job[w] = wjob[v];
        for (int l = 0; l < count[v]; l++) pl.row_idx[(size_t)w * 64 + l] = ord[first[v] + l];
    }
    // the chunks and every wave's place in the scratch of its own
    const size_t ps = (size_t)mband_smooth_strides(p, 1).ps;
    pl.wave_sc.resize((size_t)W);
    size_t used = 0;
    long nw = 0;
    for (long w = 0; w < W; w++) {
        const size_t need = (size_t)ng(pl.wave_job[w]) * ps;
        if (w == 0 || (forced > 0 && nw >= forced) || (used + need) * sizeof(double) > cap) {
            pl.chunk0.push_back(w);
            used = 0;
            nw = 0;
        }
        pl.wave_sc[w] = (long)used;
        used += need;
        nw++;
        pl.sc_max = std::max(pl.sc_max, used);
    }
    pl.chunk0.push_back(W);
    return pl;
}

}  // namespace carma

#endif
