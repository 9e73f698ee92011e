// carma_mseries_plan.h -- host-side launch planning of the multi-series calls (carma_mseries.hip, carma_mitems.hip): which wave,
// lane or lane group works on which series and item, and where its results go.  Pure functions of plain arrays that fill plain
// vectors or tables the caller owns.  Plain C++, no HIP: compiled stand-alone by tests/mseries/plan_main.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <numeric>
#include <vector>

#include "carma_smooth_plan.h"

namespace carma {

// ---- shared pieces ------------------------------------------------------------------------------------------------------
// Counting sort of M items by series index: cnt[S] items of series s, first[S + 1] its running sum, order[M] the items grouped
// by series, each group in the caller's order (pos: scratch).  A workspace the caller keeps, so that a call per optimiser step
// allocates nothing.
struct SeriesBuckets {
    std::vector<int> cnt, first, order, pos;
};

// -1, or the first i whose series[i] lies outside [0, S) (b is unspecified then)
inline long bucket_by_series(const int* series, long M, int S, SeriesBuckets& b)
{
    b.cnt.assign(S, 0);
    for (long i = 0; i < M; i++) {
        const int s = series[i];
        if (s < 0 || s >= S) return i;
        b.cnt[s]++;
    }
    b.first.assign((size_t)S + 1, 0);
    for (int s = 0; s < S; s++) b.first[s + 1] = b.first[s] + b.cnt[s];
    b.order.resize(M);
    b.pos.assign(b.first.begin(), b.first.end() - 1);
    for (long i = 0; i < M; i++) b.order[b.pos[series[i]]++] = (int)i;
    return -1;
}

// The times of item i are [toff[i], toff[i + 1]) of the caller's array.  TOFF_OK, TOFF_NEGATIVE (toff[0] < 0), or the first
// item i >= 0 with toff[i + 1] < toff[i].
constexpr long TOFF_OK = -1, TOFF_NEGATIVE = -2;
inline long check_toff(const long* toff, int M)
{
    if (toff[0] < 0) return TOFF_NEGATIVE;
    for (int i = 0; i < M; i++)
        if (toff[i + 1] < toff[i]) return i;
    return TOFF_OK;
}

// ---- carma_mpt_* --------------------------------------------------------------------------------------------------------
// Iterations per chunk of the sampler whose longest series has nmax data: the K1 of an iteration runs as long as that series
// (>= ~0.45 us per datum, as chunk_iters of the single-series lane sampler), 2-3 launches each; around a quarter of a second, at
// most 4096 iterations, are in flight at a time.
inline long mpt_chunk_iters(int nmax)
{
    const double est_us = std::max(1.0, 0.45 * nmax);
    return (long)std::max(1.0, std::min(4096.0, 250000.0 / est_us));
}

// ---- carma_mlogdensity_batch --------------------------------------------------------------------------------------------
// B evaluations, evaluation i on series[i]: waves of 64 evaluations of ONE series each, W = sum over the series of
// ceil(cnt / 64).  The series that have evaluations come with the irregular-cadence ones (repdt = 0) first -- the waves
// [0, w_plain), a launch of their own -- and within each class the longest first; ties keep the series' order.
struct MlogdensPlan {
    SeriesBuckets b;
    std::vector<int> used;            // the series with evaluations, in launch order
    long W = 0, w_plain = 0;
};

// Step 1 (O(B + S log S)): the buckets, the series order and the wave counts -- W sizes the tables of step 2.
// -1, or the first i with series[i] out of range.
inline long mlogdens_plan_count(const int* series, int B, int S, const int* nser, const char* repdt, MlogdensPlan& pl)
{
    const long bad = bucket_by_series(series, B, S, pl.b);
    if (bad >= 0) return bad;
    pl.used.clear();
    pl.W = pl.w_plain = 0;
    for (int s = 0; s < S; s++)
        if (pl.b.cnt[s]) {
            pl.used.push_back(s);
            const long w = (pl.b.cnt[s] + 63) / 64;
            pl.W += w;
            if (!repdt[s]) pl.w_plain += w;
        }
    std::stable_sort(pl.used.begin(), pl.used.end(), [&](int a, int b) {
        if (repdt[a] != repdt[b]) return repdt[a] < repdt[b];
        return nser[a] > nser[b];
    });
    return -1;
}

// Step 2: wave_series[W]; eval_idx[64 W]: lane l of wave w evaluates eval_idx[64 w + l], -1 for a pad lane (pads only trail)
inline void mlogdens_plan_fill(const MlogdensPlan& pl, int* wave_series, int* eval_idx)
{
    long w = 0;
    for (int s : pl.used)
        for (int k = pl.b.first[s]; k < pl.b.first[s + 1]; k += 64, w++) {
            wave_series[w] = s;
            int* ew = eval_idx + (size_t)w * 64;
            const int m = std::min(64, pl.b.first[s + 1] - k);
            std::memcpy(ew, &pl.b.order[k], sizeof(int) * m);
            for (int l = m; l < 64; l++) ew[l] = -1;
        }
}

// ---- carma_mkfilter -----------------------------------------------------------------------------------------------------
// M items, one per lane: the items sorted by length, longest first (ties in the caller's order) -- slot j is lane j % 64 of
// wave j / 64, and the lanes of a wave run to the wave's longest series, that of its first slot.  Wave w writes a tile of
// [2 n(first slot)][lanes of w] doubles at tile_off[w].
struct MfilterPlan {
    long M = 0, W = 0;
    std::vector<long> offs;           // [M + 1] start of item i in the caller's ragged outputs
    std::vector<int> order;           // [M] slot j holds item order[j]
    std::vector<int> tint;            // slot_series [M], slot_n [M]
    std::vector<long> tlong;          // tile_off [W], slot_out [M] (= offs of the slot's item)
    size_t tile_total = 0;            // doubles of all tiles
    long nmax = 0;                    // the longest item
};

inline MfilterPlan mfilter_plan(const int* series, int M, const int* nser)
{
    MfilterPlan pl;
    pl.M = M;
    pl.W = ((long)M + 63) / 64;
    pl.offs.assign((size_t)M + 1, 0);
    for (int i = 0; i < M; i++) pl.offs[i + 1] = pl.offs[i] + nser[series[i]];
    pl.order.resize(M);
    std::iota(pl.order.begin(), pl.order.end(), 0);
    std::stable_sort(pl.order.begin(), pl.order.end(), [&](int a, int b) { return nser[series[a]] > nser[series[b]]; });
    pl.tint.resize((size_t)2 * M);
    pl.tlong.resize((size_t)pl.W + M);
    for (long j = 0; j < M; j++) {
        const int i = pl.order[j], s = series[i];
        pl.tint[j] = s;
        pl.tint[(size_t)M + j] = nser[s];
        pl.tlong[(size_t)pl.W + j] = pl.offs[i];
        if (j % 64 == 0) {
            pl.tlong[j / 64] = (long)pl.tile_total;
            pl.tile_total += (size_t)2 * nser[s] * (size_t)std::min(64L, (long)M - j);
        }
    }
    if (M > 0) pl.nmax = nser[series[pl.order[0]]];
    return pl;
}

// ---- carma_mpredict -----------------------------------------------------------------------------------------------------
// T = toff[M] - toff[0] (item, time) pairs; output index o = position in the caller's arrays - toff[0].
//   G = 0, CAR(1): a lane per pair in the caller's order.  tint: item_series [M], pair_item [T]; W = ceil(T / 64); no tlong.
//   G >= 2: a lane group per pair, E = 64 / G groups a wave, a wave on ONE series: the pairs grouped by series (the items of a
//     series in the caller's order), the longest series first (ties in the series' order).  tint: wave_series [W], pair_item
//     [W E]; tlong: pair_out [W E], -1 for an idle group (idle groups only trail a series' last wave).
struct MpredictPlan {
    long W = 0, T = 0;
    int E = 64;
    std::vector<int> tint;
    std::vector<long> tlong;
};

// every series[i] must lie in [0, S) and toff must have passed check_toff; b: workspace
inline MpredictPlan mpredict_plan(int G, const int* series, int M, int S, const int* nser, const long* toff, SeriesBuckets& b)
{
    MpredictPlan pl;
    const long t0 = toff[0], T = toff[M] - t0;
    pl.T = T;
    pl.E = G ? 64 / G : 64;
    const int E = pl.E;
    if (!G) {
        pl.tint.resize((size_t)M + T);
        for (int i = 0; i < M; i++) {
            pl.tint[i] = series[i];
            std::fill(pl.tint.begin() + M + (toff[i] - t0), pl.tint.begin() + M + (toff[i + 1] - t0), i);
        }
        pl.W = (T + 63) / 64;
        return pl;
    }
    (void)bucket_by_series(series, M, S, b);
    std::vector<long> npair((size_t)S, 0);
    for (int i = 0; i < M; i++) npair[series[i]] += toff[i + 1] - toff[i];
    std::vector<int> used;
    for (int s = 0; s < S; s++)
        if (npair[s]) {
            used.push_back(s);
            pl.W += (npair[s] + E - 1) / E;
        }
    std::stable_sort(used.begin(), used.end(), [&](int a, int c) { return nser[a] > nser[c]; });
    const long W = pl.W;
    pl.tint.assign((size_t)W + (size_t)W * E, 0);
    pl.tlong.assign((size_t)W * E, -1L);
    long w = 0;
    for (int s : used) {
        long g = w * E;                                       // next group of this series
        for (int k = b.first[s]; k < b.first[s + 1]; k++) {
            const int i = b.order[k];
            for (long o = toff[i] - t0; o < toff[i + 1] - t0; o++, g++) {
                pl.tint[(size_t)W + g] = i;
                pl.tlong[g] = o;
            }
        }
        const long w1 = w + (npair[s] + E - 1) / E;
        for (; w < w1; w++) pl.tint[w] = s;
    }
    return pl;
}

// ---- carma_msmooth ------------------------------------------------------------------------------------------------------
// The items that have times, stably sorted by (series, number of times, the times one by one); a run of equal keys is a JOB: one
// series, one list of requested times, one merged grid (smooth_merge).  The items of a job fill waves of E slots (G >= 2: E =
// 64 / G lane groups; G = 0, CAR(1): 64 lanes); the last wave of a job is padded with idle slots (item -1, output 0).
//   tint:  wave_job [W], job_series [J], job_ng [J], slot_item [W E], src (the jobs' grids' src, concatenated)
//   tlong: job_goff [J] (start of the job's grid in grids / src), slot_out [W E] (toff[item] - toff[0]), wave_pts [W]
//   grids: the jobs' grids, concatenated
// Chunks of consecutive waves [chunk0[c], chunk0[c + 1]) share the scratch: a chunk ends before the wave that would take it
// past SMOOTH_SCRATCH_CAP (a wave of ng grid points needs smooth_wave_bytes(G, 1) ng bytes) or past `forced` models' waves
// ("SMOOTH_CHUNK_MODELS"; <= 0: no such limit).  wave_pts[w]: grid points of the waves before w in its chunk; pts_max: the most
// grid points a chunk holds.
struct MsmoothPlan {
    int E = 64;
    long W = 0, J = 0;
    std::vector<int> tint;
    std::vector<long> tlong;
    std::vector<double> grids;
    std::vector<long> chunk0;
    size_t pts_max = 0;
};

// t, hoff, nser: the sorted data times of all series, the start of series s in them, its length
inline MsmoothPlan msmooth_plan(int G, const int* series, int M, const double* tout, const long* toff, const double* t,
                                const long* hoff, const int* nser, long forced)
{
    MsmoothPlan pl;
    const int E = pl.E = G ? 64 / G : 64;
    const long t0 = toff[0];
    auto len = [&](int i) { return toff[i + 1] - toff[i]; };
    auto cmp = [&](int a, int b) {                            // <0, 0, >0
        if (series[a] != series[b]) return series[a] < series[b] ? -1 : 1;
        if (len(a) != len(b)) return len(a) < len(b) ? -1 : 1;
        for (long k = 0; k < len(a); k++) {
            const double x = tout[toff[a] + k], y = tout[toff[b] + k];
            if (x != y) return x < y ? -1 : 1;
        }
        return 0;
    };
    std::vector<int> ord;
    for (int i = 0; i < M; i++)
        if (len(i) > 0) ord.push_back(i);
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return cmp(a, b) < 0; });
    std::vector<int> wave_job, job_series, job_ng, slot_item, srcs;
    std::vector<long> job_goff, slot_out;
    for (size_t k = 0; k < ord.size();) {
        size_t k1 = k + 1;
        while (k1 < ord.size() && cmp(ord[k], ord[k1]) == 0) k1++;
        const int i0 = ord[k], s = series[i0], job = (int)job_series.size();
        const SmoothGrid sg = smooth_merge(t + hoff[s], nser[s], tout + toff[i0], (int)len(i0));
        job_series.push_back(s);
        job_ng.push_back(sg.ng);
        job_goff.push_back((long)pl.grids.size());
        pl.grids.insert(pl.grids.end(), sg.grid.begin(), sg.grid.end());
        srcs.insert(srcs.end(), sg.src.begin(), sg.src.end());
        for (size_t a = k; a < k1; a += E) {
            wave_job.push_back(job);
            for (size_t b = a; b < a + E; b++) {
                slot_item.push_back(b < k1 ? ord[b] : -1);
                slot_out.push_back(b < k1 ? toff[ord[b]] - t0 : 0L);
            }
        }
        k = k1;
    }
    const long W = pl.W = (long)wave_job.size();
    pl.J = (long)job_series.size();
    const long wmax = forced > 0 ? (forced + E - 1) / E : W;
    std::vector<long> wave_pts((size_t)W);
    size_t pts = 0;
    long nw = 0;
    for (long w = 0; w < W; w++) {
        const size_t ng = (size_t)job_ng[wave_job[w]];
        if (w == 0 || nw >= wmax || smooth_wave_bytes(G, 1) * (pts + ng) > SMOOTH_SCRATCH_CAP) {
            pl.chunk0.push_back(w);
            pts = 0;
            nw = 0;
        }
        wave_pts[w] = (long)pts;
        pts += ng;
        nw++;
        pl.pts_max = std::max(pl.pts_max, pts);
    }
    pl.chunk0.push_back(W);
    for (const std::vector<int>* v : {&wave_job, &job_series, &job_ng, &slot_item, &srcs}) pl.tint.insert(pl.tint.end(), v->begin(), v->end());
    for (const std::vector<long>* v : {&job_goff, &slot_out, &wave_pts}) pl.tlong.insert(pl.tlong.end(), v->begin(), v->end());
    return pl;
}

}  // namespace carma
