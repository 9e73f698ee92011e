// carma_smooth_plan.h -- host-side planning of the one-pass smoother (carma_smooth.hip): the merged grid of data and requested
// times with its position tables, the strides of the scratch records and the chunk sizes.  Plain C++, no HIP: compiled
// stand-alone by tests/smooth/plan_main.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <numeric>
#include <vector>

namespace carma {

constexpr size_t SMOOTH_SCRATCH_CAP = (size_t)256 << 20;    // bytes of scratch records per chunk (the conditional simulation's cap)

// The grid both passes walk: point i is a datum or a requested time, ascending; a requested time equal to a datum comes behind
// it and equal requested times keep the caller's order (a step of dt = 0 is exact, so ties may go either way).
//   grid[ng]  the times, ng = n + M
//   dpos[n]   position of datum j
//   spos[M]   position of requested time i (the caller's order)
//   src[ng]   what point i is: datum j >= 0, or -1 - i for requested time i
struct SmoothGrid {
    int n = 0, M = 0, ng = 0;
    std::vector<double> grid;
    std::vector<int> dpos, spos, src;
};

// t: the n sorted, distinct data times; tout: the M requested times in any order, repeats allowed
inline SmoothGrid smooth_merge(const double* t, int n, const double* tout, int M)
{
    SmoothGrid g;
    g.n = n;
    g.M = M;
    g.ng = n + M;
    std::vector<int> perm(M);                                 // sorted tout r = caller's tout perm[r]
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return tout[a] < tout[b]; });
    std::vector<double> cat(g.ng);
    for (int j = 0; j < n; j++) cat[j] = t[j];
    for (int r = 0; r < M; r++) cat[n + r] = tout[perm[r]];
    std::vector<int> order(g.ng);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cat[a] < cat[b]; });
    g.grid.resize(g.ng);
    g.src.resize(g.ng);
    g.dpos.resize(n);
    g.spos.resize(M);
    for (int i = 0; i < g.ng; i++) {
        const int s = order[i];
        g.grid[i] = cat[s];
        if (s < n) {
            g.src[i] = s;
            g.dpos[s] = i;
        } else {
            g.src[i] = -1 - perm[s - n];
            g.spos[perm[s - n]] = i;
        }
    }
    return g;
}

// Scratch of one chunk.  CARMA(p >= 2), G lanes per model: a wave holds E = 64 / G models; per point it stores 64 lane records
// {u.re, u.im, rho.re, rho.im} (2 KiB, contiguous) and E group records {1/F or 0, v, Sx, f}: record of (wave w, point i, lane l)
// at double4 index (w ng + i) 64 + l, group record of (w, i, group e) at (w ng + i) E + e.  That is 32 G + 32 bytes per point
// and model.  CAR(1) (G = 0 here): one lane per model, E = 64, five planes of doubles {phi, 1/F or 0, v, x, f}: value q of
// (lane L of the chunk, point i) at (q ng + i) lanes + L with lanes = 64 waves; 40 bytes per point and model.
struct SmoothChunks {
    int E = 0;                // models per wave
    long models = 0;          // models per chunk (the last chunk may hold fewer)
    long waves = 0;           // waves (= workgroups) of a full chunk
    size_t rec_elems = 0;     // double4 lane records of a chunk (CAR(1): doubles of all planes)
    size_t grp_elems = 0;     // double4 group records of a chunk (CAR(1): 0)
    size_t bytes = 0;         // both together
};

inline size_t smooth_wave_bytes(int G, int ng)
{
    const int E = G ? 64 / G : 64;
    return G ? (size_t)ng * (64 * 32 + (size_t)E * 32) : (size_t)ng * 64 * 40;
}

// forced: models per chunk asked for ("SMOOTH_CHUNK_MODELS"; <= 0: automatic, as many whole waves as the cap holds, one at least)
inline SmoothChunks smooth_chunks(int G, int ng, long nmodels, long forced, size_t cap = SMOOTH_SCRATCH_CAP)
{
    SmoothChunks c;
    c.E = G ? 64 / G : 64;
    const size_t wb = std::max<size_t>(1, smooth_wave_bytes(G, ng));
    long models = forced > 0 ? forced : (long)std::max<size_t>(1, cap / wb) * c.E;
    models = std::max(1L, std::min(models, std::max(1L, nmodels)));
    c.models = models;
    c.waves = (models + c.E - 1) / c.E;
    if (G) {
        c.rec_elems = (size_t)c.waves * ng * 64;
        c.grp_elems = (size_t)c.waves * ng * c.E;
        c.bytes = 32 * (c.rec_elems + c.grp_elems);
    } else {
        c.rec_elems = (size_t)c.waves * 64 * ng * 5;
        c.grp_elems = 0;
        c.bytes = 8 * c.rec_elems;
    }
    return c;
}

}  // namespace carma
