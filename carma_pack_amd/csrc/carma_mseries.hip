// carma_mseries.hip -- MANY series in one launch: the one-evaluation-per-lane log-density kernels with the series chosen per
// wave from a table, the launch plan that builds that table, and the multi-series context of the C ABI (carma_mctx_*).
//
// A survey fits thousands of light curves, each on its own; a launch per series leaves most of the chip idle (one series
// rarely supplies the ~25 000 evaluations the lane kernel needs to fill 256 CUs).  Here all series of a set live in ONE
// buffer in HBM and a launch carries evaluations of any of them:
//   - one wave per workgroup, as k_logdens_carma_lane; wave w works on series wave_series[w] -- an index that derives from
//     blockIdx.x alone, so the series' offset, length and prior bounds are wave-uniform and come in with scalar loads, and so
//     do the series records in the filter loop, exactly as in the single-series kernel;
//   - lane l of wave w evaluates parameter vector eval_idx[64 w + l] and writes out[eval_idx[64 w + l]] (the caller's order);
//     pad lanes (eval_idx = -1) compute a copy of the wave's first evaluation and write nothing;
//   - the filter is logdensity_lane / logdensity_car1 unchanged, and REPDT is decided per series as carma_ctx_create decides
//     it: a series gives the same bits as the single-series lane kernel on it.
//
// Filter() and Predict of MANY (series, model) items in one launch (carma_mkfilter, carma_mpredict):
//   - filter: one ITEM per lane -- kfilter_lane / car1_filter with a series pointer and a length of the lane's own.  The loop over
//     the data is a divergent one (a lane that has finished is masked off by the compiler's exec handling; nothing inside
//     lane_filter with in-line factors talks across lanes), the records come in with per-lane vector loads, and the host plan
//     sorts the items by length so that a wave's lanes finish together.  A wave writes into a tile of its own, [2 nmax_w][lanes]
//     (row k: mean_k of every lane; row n_l + k: var_k of lane l), so that the stores of a step are contiguous wherever the
//     lanes' lengths agree; k_mtranspose_mv then moves the tiles into the caller's ragged layout, 32 data of an item at a time;
//   - predict: one lane GROUP per (item, time) with predict_run; its group exchange needs one trip count per wave, so a wave
//     takes ONE series (wave table indexed by blockIdx.x) and its 64 / G groups take (item, time) pairs on that series.
//
// The SAMPLER over many series (carma_mpt_*): the large-ensemble sampler of carma_pt_lane.hip -- one chain per
// lane, an iteration as k_ram_propose / K1 / k_ram_finish -- with a K1 in which every chain is evaluated on the series of its own
// ladder (k_logdens_carma_chains_ms).  A RUN is one sampler (R replicas x T temperatures) on one series; a call's M runs are the
// ladders j R .. j R + R - 1 of ONE ensemble of M R ladders, so the bookkeeping kernels, the Philox keys and the start-value keys
// are those of a single-series ensemble of that size, and run j is its block replica0 = j R.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "../../include/carma_mi355.h"
#include "grp_device.h"
#include "carma_core.h"
#include "carma_host.h"
#include "carma_lane.h"
#include "carma_predict.h"
#include "carma_pt_sched.h"
#include "carma_smooth.h"
#include "carma_smooth_plan.h"

namespace carma {

template <int P, bool REPDT>
__global__ __launch_bounds__(64) void k_logdens_carma_lane_ms(const double* __restrict__ theta, int d, int q,
                                                             const double4* __restrict__ records, const long* __restrict__ off,
                                                             const int* __restrict__ nser, const Prior* __restrict__ prs,
                                                             const int* __restrict__ wave_series, const int* __restrict__ eval_idx,
                                                             int ignore_prior, double* __restrict__ out)
{
    __shared__ double s_tab[MATH_TAB_N];                     // tables of the table-based exp / sincos (carma_math.h)
    math_tab_fill(s_tab);
    __syncthreads();
    const int s = wave_series[blockIdx.x];                   // wave-uniform: scalar loads of the series' record
    const double4* series = records + off[s];
    const int n = nser[s];
    const Prior pr = prs[s];
    const int* ew = eval_idx + (long)blockIdx.x * 64;
    int e = ew[threadIdx.x];
    const bool live = e >= 0;
    if (!live) e = ew[0];                                    // (lane 0 of a wave is always live)
    const double ll = logdensity_lane<P, REPDT>(theta + (long)e * d, q, series, n, pr, ignore_prior, s_tab);
    if (live) out[e] = ll;
}

__global__ __launch_bounds__(64) void k_logdens_car1_ms(const double* __restrict__ theta, const double4* __restrict__ records,
                                                        const long* __restrict__ off, const int* __restrict__ nser,
                                                        const Prior* __restrict__ prs, const int* __restrict__ wave_series,
                                                        const int* __restrict__ eval_idx, double* __restrict__ out)
{
    const int s = wave_series[blockIdx.x];
    const double4* series = records + off[s];
    const int n = nser[s];
    const Prior pr = prs[s];
    const int* ew = eval_idx + (long)blockIdx.x * 64;
    int e = ew[threadIdx.x];
    const bool live = e >= 0;
    if (!live) e = ew[0];
    const double ll = logdensity_car1(theta + 4L * e, series, n, pr);
    if (live) out[e] = ll;
}

// nwaves waves of the table (wave_series[nwaves], eval_idx[64 nwaves]) in one launch
static hipError_t launch_logdens_ms(int p, bool repdt, const double* theta, int d, int q, const double4* records, const long* off,
                                    const int* nser, const Prior* prs, const int* wave_series, const int* eval_idx, long nwaves,
                                    int ignore_prior, double* out, hipStream_t st)
{
    if (nwaves <= 0) return hipSuccess;
    const dim3 grid((unsigned)nwaves), block(64);
    if (p == 1) {
        hipLaunchKernelGGL(k_logdens_car1_ms, grid, block, 0, st, theta, records, off, nser, prs, wave_series, eval_idx, out);
        return hipGetLastError();
    }
    switch (p) {
#define CARMA_MS(N)                                                                                                            \
    case N:                                                                                                                    \
        if (repdt)                                                                                                             \
            hipLaunchKernelGGL((k_logdens_carma_lane_ms<N, true>), grid, block, 0, st, theta, d, q, records, off, nser, prs,   \
                               wave_series, eval_idx, ignore_prior, out);                                                      \
        else                                                                                                                   \
            hipLaunchKernelGGL((k_logdens_carma_lane_ms<N, false>), grid, block, 0, st, theta, d, q, records, off, nser, prs,  \
                               wave_series, eval_idx, ignore_prior, out);                                                      \
        break;
        CARMA_MS(2) CARMA_MS(3) CARMA_MS(4) CARMA_MS(5) CARMA_MS(6) CARMA_MS(7)
#undef CARMA_MS
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// K1 of the multi-series sampler: ONE CHAIN PER LANE, chain gi = 64 blockIdx.x + threadIdx.x of the ensemble, on the series of its
// ladder, ladder_series[gi / T].  thn = [nc][d] chain-major (the proposals k_ram_propose / k_ram_finish write), ll = [nc].
//   - the series' offset, length and prior are per-lane values and the records come in with per-lane vector loads (the lanes of a
//     ladder share an address); the loop over the data is a divergent one that ends at the wave's longest series;
//   - logdensity_lane has ONE wave-wide operation, the ballot "does any lane have a real pair" in front of the loop, and what it
//     guards only ever changes lanes that have such a pair: its outcome cannot change a lane's bits, whatever the lanes' lengths;
//   - REPDT is a property of the SERIES (rep[s], as carma_ctx_create decides it) and selects another instruction stream, so the
//     regular-cadence series' chains are served by a launch of their own: a lane whose series belongs to the other launch leaves
//     (after the barrier), a wave without any lane of this launch is gone at once.  A chain gets the bits of the single-series lane
//     kernel on its series, as k_logdens_carma_lane_ms gives them;
//   - lanes past nc shadow the last chain and write nothing.
template <int P, bool REPDT>
__global__ __launch_bounds__(64) void k_logdens_carma_chains_ms(const double* __restrict__ thn, int d, int q, long nc, int T,
                                                               const double4* __restrict__ records, const long* __restrict__ off,
                                                               const int* __restrict__ nser, const Prior* __restrict__ prs,
                                                               const char* __restrict__ rep, const int* __restrict__ ladder_series,
                                                               double* __restrict__ ll)
{
    __shared__ double s_tab[MATH_TAB_N];                     // tables of the table-based exp / sincos (carma_math.h)
    math_tab_fill(s_tab);
    __syncthreads();
    long gi = (long)blockIdx.x * 64 + threadIdx.x;
    const bool live = gi < nc;
    if (!live) gi = nc - 1;
    const int s = ladder_series[gi / T];
    if ((rep[s] != 0) != REPDT) return;
    const double v = logdensity_lane<P, REPDT>(thn + gi * d, q, records + off[s], nser[s], prs[s], 0, s_tab);
    if (live) ll[gi] = v;
}

__global__ __launch_bounds__(64) void k_logdens_car1_chains_ms(const double* __restrict__ thn, long nc, int T,
                                                              const double4* __restrict__ records, const long* __restrict__ off,
                                                              const int* __restrict__ nser, const Prior* __restrict__ prs,
                                                              const int* __restrict__ ladder_series, double* __restrict__ ll)
{
    long gi = (long)blockIdx.x * 64 + threadIdx.x;
    const bool live = gi < nc;
    if (!live) gi = nc - 1;
    const int s = ladder_series[gi / T];
    const double v = logdensity_car1(thn + 4 * gi, records + off[s], nser[s], prs[s]);
    if (live) ll[gi] = v;
}

// Filter() of M items, one per lane.  par: per slot [M][3 P + 2] as k_kfilter_carma_lane takes it, slots in the plan's order (longest
// series first); slot_series[M]; tile_off[waves]: start of the wave's tile in mv.  Lanes past M leave after the barrier.
template <int P>
__global__ __launch_bounds__(64) void k_mkfilter_carma_lane(const double* __restrict__ par, int M, const double4* __restrict__ records,
                                                           const long* __restrict__ off, const int* __restrict__ nser,
                                                           const int* __restrict__ slot_series, const long* __restrict__ tile_off,
                                                           double* __restrict__ mv, int* __restrict__ singular)
{
    __shared__ double s_tab[MATH_TAB_N];
    math_tab_fill(s_tab);
    __syncthreads();
    const long slot = (long)blockIdx.x * 64 + threadIdx.x;
    if (slot >= M) return;
    const long ld = min(64L, (long)M - (long)blockIdx.x * 64);            // lanes of this wave that hold an item
    const int s = slot_series[slot];
    const double* pm = par + slot * (3 * P + 2);
    const bool sing = kfilter_lane<P>(pm, pm + 2 * P, pm[3 * P], pm[3 * P + 1], records + off[s], nser[s], s_tab,
                                      mv + tile_off[blockIdx.x] + threadIdx.x, ld);
    singular[slot] = sing ? 1 : 0;
}

// CAR(1): par = [M][3] (sigsqr, omega, mu), the same tiles
__global__ __launch_bounds__(64) void k_mkfilter_car1(const double* __restrict__ par, int M, const double4* __restrict__ records,
                                                      const long* __restrict__ off, const int* __restrict__ nser,
                                                      const int* __restrict__ slot_series, const long* __restrict__ tile_off,
                                                      double* __restrict__ mv)
{
    const long slot = (long)blockIdx.x * 64 + threadIdx.x;
    if (slot >= M) return;
    const long ld = min(64L, (long)M - (long)blockIdx.x * 64);
    const int s = slot_series[slot];
    const int n = nser[s];
    const double* pm = par + slot * 3;
    double* t = mv + tile_off[blockIdx.x] + threadIdx.x;
    (void)car1_filter(pm[0], pm[1], pm[2], 1.0, records + off[s], n, true, t, t + (long)n * ld, ld, true);
}

// The tiles of the filter kernels -> the caller's ragged arrays: the item in lane l of wave blockIdx.x has slot_n data, its
// means go to mean[slot_out + k], its variances to var[slot_out + k].  32 rows of a tile at a time through LDS: the reads
// follow the tile's rows, the writes put 32 consecutive data of one item side by side; nothing is written at or past k = n_l.
__global__ __launch_bounds__(256) void k_mtranspose_mv(const double* __restrict__ mv, const long* __restrict__ tile_off, int M,
                                                       const int* __restrict__ slot_n, const long* __restrict__ slot_out,
                                                       double* __restrict__ mean, double* __restrict__ var)
{
    __shared__ double s_m[32][65], s_v[32][65];
    __shared__ int s_n[64];
    __shared__ long s_o[64];
    const long slot0 = (long)blockIdx.x * 64;
    const int ld = (int)min(64L, (long)M - slot0);
    if (threadIdx.x < 64) {
        const bool live = (int)threadIdx.x < ld;
        s_n[threadIdx.x] = live ? slot_n[slot0 + threadIdx.x] : 0;
        s_o[threadIdx.x] = live ? slot_out[slot0 + threadIdx.x] : 0;
    }
    __syncthreads();
    const int nmax = s_n[0];                                  // the plan sorts by length: lane 0 holds the wave's longest
    const double* tile = mv + tile_off[blockIdx.x];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;   // reading: 64 lanes x 4 rows
    const int kx = threadIdx.x & 31, ly = threadIdx.x >> 5;   // writing: 32 data x 8 items
    for (int k0 = blockIdx.y * 32; k0 < nmax; k0 += gridDim.y * 32) {
        const int ntx = s_n[tx];
        for (int j = ty; j < 32; j += 4) {
            const int k = k0 + j;
            if (k < ntx) {
                s_m[j][tx] = tile[(long)k * ld + tx];
                s_v[j][tx] = tile[((long)ntx + k) * ld + tx];
            }
        }
        __syncthreads();
        const int k = k0 + kx;
        for (int l = ly; l < ld; l += 8) {
            if (k < s_n[l]) {
                mean[s_o[l] + k] = s_m[kx][l];
                var[s_o[l] + k] = s_v[kx][l];
            }
        }
        __syncthreads();
    }
}

// Predict of (item, time) pairs: wave blockIdx.x works on series wave_series[blockIdx.x], its 64 / G groups on the pairs
// pair_out[64 / G * blockIdx.x + group] (index into tpred / pmean / pvar; -1: an idle group, which repeats the wave's first
// pair and writes nothing) of item pair_item[.].  par = [items][3 P + 2] in the caller's order.
template <int P, int G>
__global__ __launch_bounds__(64) void k_mpredict_carma(const double* __restrict__ par, const double4* __restrict__ records,
                                                      const long* __restrict__ off, const int* __restrict__ nser,
                                                      const int* __restrict__ wave_series, const int* __restrict__ pair_item,
                                                      const long* __restrict__ pair_out, const double* __restrict__ tpred,
                                                      double* __restrict__ pmean, double* __restrict__ pvar, int* __restrict__ singular)
{
    __shared__ double4 xch[64];
    __shared__ double2 xch2[64];
    const int tid = threadIdx.x;
    Grp<G> g{xch, tid & 63, xch2};
    const int s = wave_series[blockIdx.x];                    // wave-uniform: one trip count for every group (predict_run's exchange)
    const double4* series = records + off[s];
    const int n = nser[s];
    long e = (long)blockIdx.x * (64 / G) + tid / G;
    const bool live = pair_out[e] >= 0;
    if (!live) e = (long)blockIdx.x * (64 / G);               // (group 0 of a wave is always live)
    const int item = pair_item[e];
    const long o = pair_out[e];
    const double* pm = par + (long)item * (3 * P + 2);
    Model<P> m;
    model_from_roots<P, G>(g, pm, pm + 2 * P, pm[3 * P], m);
    double mean, var;
    bool sing;
    predict_run<P, G>(g, m, series, n, tpred[o], &mean, &var, &sing, pm[3 * P + 1]);
    if (live && g.lane() == 0) {
        pmean[o] = mean;
        pvar[o] = var;
        if (sing) singular[item] = 1;
    }
}

// CAR(1): one lane per (item, time) pair, pairs in the caller's order; par = [items][3] (sigsqr, omega, mu)
__global__ __launch_bounds__(64) void k_mpredict_car1(const double* __restrict__ par, const double4* __restrict__ records,
                                                      const long* __restrict__ off, const int* __restrict__ nser,
                                                      const int* __restrict__ item_series, const int* __restrict__ pair_item,
                                                      long npairs, const double* __restrict__ tpred, double* __restrict__ pmean,
                                                      double* __restrict__ pvar)
{
    const long e = (long)blockIdx.x * 64 + threadIdx.x;
    if (e >= npairs) return;
    const int item = pair_item[e];
    const int s = item_series[item];
    const double* pm = par + 3L * item;
    predict_car1(pm[0], pm[1], records + off[s], nser[s], tpred[e], pmean + e, pvar + e, pm[2]);
}

// Sampler state of a multi-series context (carma_mpt_*): M runs of `reps` ladders of T chains = one ensemble of R = M reps ladders
struct MptState : PtEnsemble {
    int M = 0, reps = 0;              // runs, replicas per run
    std::vector<int> series;          // [M] series of run j
    int nmax = 0;                     // the longest series of the call
    bool any_plain = false, any_rep = false;   // the call holds irregular / regular-cadence series
    int* d_lser = nullptr;            // [R] series of every ladder, uploaded once
    char* d_rep = nullptr;            // [S] SERIES_REPEATED_DT of every series
};

// Multi-series context: the series of a set packed one after another in HBM, each as carma_ctx_create packs one
struct Mctx {
    MptState* mpt = nullptr;
    int device = 0;
    int p = 0, q = 0, d = 0, S = 0;
    std::vector<long> hoff;           // [S + 1] start of series s in t / y / yerr (after sort/dedup)
    std::vector<double> t, y, yerr;   // all series, sorted and deduplicated, concatenated
    std::vector<long> off;            // [S] first record of series s in d_rec (a multiple of 2 records: 64-byte aligned)
    std::vector<int> n;               // [S]
    std::vector<Prior> pr;            // [S]
    std::vector<char> repdt;          // [S] SERIES_REPEATED_DT of each series
    DevMem d_rec, d_off, d_n, d_pr;   // records of all series; [S] each: off, n, pr
    const double4* rec() const { return d_rec.as<const double4>(); }
    const long* offs() const { return d_off.as<const long>(); }
    const int* ns() const { return d_n.as<const int>(); }
    const Prior* prs() const { return d_pr.as<const Prior>(); }
    // per-call buffers, grown on demand: parameter vectors [cap_B][d], results [cap_B], plan [cap_W] + [cap_W][64]
    DevMem d_theta, d_out, d_wser, d_eidx;
    char* h_stage = nullptr;          // pinned: the same four, in this order
    long cap_B = 0, cap_W = 0;
    hipStream_t stream = nullptr;
    std::vector<int> cnt, first, order, wser_tmp;
    // carma_mkfilter / carma_mpredict: parameters and times (doubles), plan tables (ints, longs), tiles, results, flags; grown by
    // DevMem::need
    DevMem k_par, k_int, k_long, k_tile, k_res, k_sing;

    size_t stage_bytes(long B, long W) const { return sizeof(double) * (size_t)B * (d + 1) + sizeof(int) * (size_t)W * 65; }
    int ensure(long B, long W)
    {
        if (B <= cap_B && W <= cap_W) return CARMA_OK;
        const long nB = std::max(std::max(B, cap_B), 1024L), nW = std::max(std::max(W, cap_W), 64L);
        for (DevMem* b : {&d_theta, &d_out, &d_wser, &d_eidx}) b->release();
        if (h_stage) (void)hipHostFree(h_stage);
        h_stage = nullptr;
        cap_B = cap_W = 0;
        hipError_t e = d_theta.alloc(sizeof(double) * (size_t)nB * d);
        if (e == hipSuccess) e = d_out.alloc(sizeof(double) * (size_t)nB);
        if (e == hipSuccess) e = d_wser.alloc(sizeof(int) * (size_t)nW);
        if (e == hipSuccess) e = d_eidx.alloc(sizeof(int) * (size_t)nW * 64);
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&h_stage), stage_bytes(nB, nW), hipHostMallocDefault);
        if (e != hipSuccess) return hip_fail(e, "carma_mlogdensity_batch: buffers");
        cap_B = nB;
        cap_W = nW;
        return CARMA_OK;
    }
};

// The items of carma_mkfilter / carma_mpredict -> par [M][3 p + 2] (p = 1: [M][3]: sigsqr, omega, mu) in the caller's order, as
// the kernels read them.  Host only; an argument error names its item.
static int pack_items(const Mctx* c, const char* who, const int* series, int M, const double* sigsqr, const double* om,
                      const double* ma, int nma, const double* mu, std::vector<double>& par)
{
    const int p = c->p;
    if (M < 1 || !series || !sigsqr || !om || (p > 1 && (!ma || nma < 1 || nma > p))) {
        set_error("%s: bad argument (M >= 1, non-null arrays, 1 <= nma <= p; got M=%d nma=%d p=%d)", who, M, nma, p);
        return CARMA_EINVAL;
    }
    const int PW = p == 1 ? 3 : 3 * p + 2;
    par.assign((size_t)M * PW, 0.0);
    for (int i = 0; i < M; i++) {
        if (series[i] < 0 || series[i] >= c->S) {
            set_error("%s: item %d: series index %d out of range (nseries = %d)", who, i, series[i], c->S);
            return CARMA_EINVAL;
        }
        if (p == 1) {
            double* pb = par.data() + (size_t)i * PW;
            if (om[2 * (size_t)i + 1] != 0.0) {
                set_error("%s: item %d: the root of a CAR(1) model must be real", who, i);
                return CARMA_EINVAL;
            }
            pb[0] = sigsqr[i];
            pb[1] = -om[2 * (size_t)i];
            pb[2] = mu ? mu[i] : 0.0;
            continue;
        }
        if (pack_model_row(p, om + (size_t)i * 2 * p, ma + (size_t)i * nma, nma, sigsqr[i], mu ? mu[i] : 0.0,
                           par.data() + (size_t)i * PW) != CARMA_OK) {
            set_error("%s: item %d: the AR roots must be real or come in complex-conjugate pairs", who, i);
            return CARMA_EINVAL;
        }
    }
    return CARMA_OK;
}

template <class T>
static hipError_t upload(DevMem& b, const std::vector<T>& v, hipStream_t st)
{
    hipError_t e = b.need(sizeof(T) * v.size());
    if (e == hipSuccess) e = hipMemcpyAsync(b.as<void>(), v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, st);
    return e;
}

// ---- the one-pass smoother over many (series, model) items (carma_msmooth) -----------------------------------------------
// A JOB is a (series, list of requested times) pair with its merged grid (carma_smooth_plan.h); the items that share a job fill
// waves of E = 64 / G groups (CAR(1): 64 lanes), so that a wave's loop over the grid is uniform; other items get waves of their
// own.  Wave w0 + blockIdx.x of the plan: job wave_job[w]; slot e of it: item slot_item[w E + e] (-1: idle, repeats the wave's
// first item and stores no output), outputs at slot_out[w E + e]; its scratch starts wave_pts[w] grid points into the chunk's.
// The device functions and the series records are those of carma_smooth_*: an item gets the bits of that call on its series.
struct MsmoothTabs {
    const int *wave_job, *job_series, *job_ng, *slot_item, *src;
    const long *job_goff, *slot_out, *wave_pts;
    const double* grid;
};

template <int P, int G>
__global__ __launch_bounds__(64) void k_msmooth_carma(const double* __restrict__ par, const double4* __restrict__ records,
                                                      const long* __restrict__ off, MsmoothTabs tb, long w0,
                                                      double4* __restrict__ rec, double4* __restrict__ grp,
                                                      double* __restrict__ mean, double* __restrict__ var,
                                                      int* __restrict__ singular)
{
    __shared__ double4 xch[64];
    __shared__ double2 xch2[64];
    constexpr int E = 64 / G;
    const int tid = threadIdx.x;
    Grp<G> g{xch, tid & 63, xch2};
    const long w = w0 + blockIdx.x;
    const int j = tb.wave_job[w];
    const double4* series = records + off[tb.job_series[j]];
    const int ng = tb.job_ng[j];
    const double* grid = tb.grid + tb.job_goff[j];
    const int* src = tb.src + tb.job_goff[j];
    const int e = tid / G;
    int item = tb.slot_item[w * E + e];
    const bool live = item >= 0;
    if (!live) item = tb.slot_item[w * E];                    // (slot 0 of a wave is always live)
    const double* pm = par + (long)item * (3 * P + 2);
    Model<P> m;
    model_from_roots<P, G>(g, pm, pm + 2 * P, pm[3 * P], m);
    const double mu = pm[3 * P + 1];
    FilterConsts<P> fc;
    filter_reset<P, G>(g, m, fc);
    double4* myrec = rec + (size_t)tb.wave_pts[w] * 64 + tid;
    double4* mygrp = grp + (size_t)tb.wave_pts[w] * E + e;
    smooth_forward<P, G>(g, m, fc, series, grid, src, ng, mu, myrec, 64, mygrp, E);
    __syncthreads();                                          // lane 0 wrote the group records, every lane of the group reads them
    const long o = tb.slot_out[w * E + e];
    smooth_backward<P, G>(g, fc, src, ng, mu, myrec, 64, mygrp, E, live ? mean + o : nullptr, live ? var + o : nullptr);
    if (live && g.lane() == 0) singular[item] = fc.sing ? 1 : 0;
}

// CAR(1): one lane per item; the wave's scratch is five planes of ng x 64 doubles
__global__ __launch_bounds__(64) void k_msmooth_car1(const double* __restrict__ par, const double4* __restrict__ records,
                                                     const long* __restrict__ off, MsmoothTabs tb, long w0, double* __restrict__ sc,
                                                     double* __restrict__ mean, double* __restrict__ var)
{
    const long w = w0 + blockIdx.x;
    const int j = tb.wave_job[w];
    const double4* series = records + off[tb.job_series[j]];
    const int ng = tb.job_ng[j];
    int item = tb.slot_item[w * 64 + threadIdx.x];
    const bool live = item >= 0;
    if (!live) item = tb.slot_item[w * 64];
    const double* pm = par + 3L * item;
    const long o = tb.slot_out[w * 64 + threadIdx.x];
    smooth_car1(pm[0], pm[1], pm[2], series, tb.grid + tb.job_goff[j], tb.src + tb.job_goff[j], ng,
                sc + (size_t)tb.wave_pts[w] * 64 * 5 + threadIdx.x, 64, 64L * ng, live ? mean + o : nullptr, live ? var + o : nullptr);
}

// ---- the sampler over many series -------------------------------------------------------------------------------------
// K1: every chain of the ensemble on its ladder's series; the regular-cadence series' chains in a launch of their own
static hipError_t launch_logdens_chains_ms(const Mctx* c, const MptState* s, const double* thn, long nc, double* ll, hipStream_t st)
{
    (void)hipGetLastError();   // HIP's last-error is sticky: drop anything left by earlier calls
    const dim3 grid((unsigned)((nc + 63) / 64)), block(64);
    if (c->p == 1) {
        hipLaunchKernelGGL(k_logdens_car1_chains_ms, grid, block, 0, st, thn, nc, s->T, c->rec(), c->offs(), c->ns(), c->prs(),
                           s->d_lser, ll);
        return hipGetLastError();
    }
    for (int rep = 0; rep < 2; rep++) {
        if (!(rep ? s->any_rep : s->any_plain)) continue;
        switch (c->p) {
#define CARMA_MCH(N)                                                                                                              \
    case N:                                                                                                                       \
        if (rep)                                                                                                                  \
            hipLaunchKernelGGL((k_logdens_carma_chains_ms<N, true>), grid, block, 0, st, thn, c->d, c->q, nc, s->T, c->rec(),     \
                               c->offs(), c->ns(), c->prs(), s->d_rep, s->d_lser, ll);                                            \
        else                                                                                                                      \
            hipLaunchKernelGGL((k_logdens_carma_chains_ms<N, false>), grid, block, 0, st, thn, c->d, c->q, nc, s->T, c->rec(),    \
                               c->offs(), c->ns(), c->prs(), s->d_rep, s->d_lser, ll);                                            \
        break;
            CARMA_MCH(2) CARMA_MCH(3) CARMA_MCH(4) CARMA_MCH(5) CARMA_MCH(6) CARMA_MCH(7)
#undef CARMA_MCH
            default: return hipErrorInvalidValue;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

static void mpt_free(Mctx* c)
{
    if (!c->mpt) return;
    pt_ens_release(c->mpt);
    if (c->mpt->d_lser) (void)dev_free(c->mpt->d_lser);
    if (c->mpt->d_rep) (void)dev_free(c->mpt->d_rep);
    delete c->mpt;
    c->mpt = nullptr;
}

// the sampler state of h, or null with the error set: `who` was called before carma_mpt_create (need_start: or before the
// chains have starting values)
static MptState* mpt_state(carma_mctx* h, const char* who, bool need_start)
{
    if (!h) {
        set_error("%s: null context", who);
        return nullptr;
    }
    MptState* s = reinterpret_cast<Mctx*>(h)->mpt;
    if (!s) {
        set_error("%s: call carma_mpt_create first", who);
        return nullptr;
    }
    if (need_start && !s->started) {
        set_error("%s: chains have no starting values (carma_mpt_start / carma_mpt_set_chains)", who);
        return nullptr;
    }
    return s;
}

// Iterations per chunk: the K1 of an iteration runs as long as its longest series (>= ~0.45 us per datum, as chunk_iters of the
// single-series lane sampler), 2-3 launches each; around a quarter of a second, at most 4096 iterations, are in flight at a time.
static long mpt_chunk_iters(const MptState* s)
{
    const double est_us = std::max(1.0, 0.45 * s->nmax);
    return (long)std::max(1.0, std::min(4096.0, 250000.0 / est_us));
}

// niter iterations, a chunk in flight at a time.  thin > 0: save the coldest chains every thin iterations from sample *save_offset on
static int mpt_iterate(Mctx* c, long niter, int do_exchange, int thin, long* save_offset)
{
    MptState* s = c->mpt;
    const long chunk0 = mpt_chunk_iters(s);
    const PtLaneK1 k1 = [c, s](const double* thn, long nc, double* ll, hipStream_t st) {
        return launch_logdens_chains_ms(c, s, thn, nc, ll, st);
    };
    long left = niter;
    while (left > 0) {
        const long ch = pt_next_chunk(left, chunk0, thin);
        const PtLaunch L = pt_ens_launch(s, c->d, c->q, s->nmax, ch, do_exchange, thin, save_offset ? *save_offset : 0);
        hipError_t e = launch_pt_lane_k1(c->p, L, s->d_scratch, k1, s->d_temps, s->d_theta, s->d_lp, s->d_chol, s->d_nacc, s->d_nswap,
                                         s->d_samples, s->d_slp, !s->factor_loaded, c->stream);
        if (e == hipSuccess) {
            s->factor_loaded = true;
            s->chol_stale = true;
            e = hipStreamSynchronize(c->stream);
        }
        if (e != hipSuccess) return hip_fail(e, "carma_mpt: sampler launch");
        pt_ens_advance(s, ch, thin, save_offset);
        left -= ch;
    }
    return CARMA_OK;
}

}  // namespace carma

using namespace carma;

extern "C" {

carma_mctx* carma_mctx_create(const double* time, const double* y, const double* yerr, const long* offsets, int nseries, int p,
                              int q, const double* max_stdev, int device)
{
    if (!time || !y || !yerr || !offsets || nseries < 1) {
        set_error("carma_mctx_create: need nseries >= 1 and non-null arrays (got nseries=%d)", nseries);
        return nullptr;
    }
    if (p < 1 || p > CARMA_PMAX || q < 0 || (p == 1 && q != 0) || (p > 1 && q >= p)) {
        set_error("carma_mctx_create: need 1 <= p <= %d and q < p (got p=%d q=%d)", CARMA_PMAX, p, q);
        return nullptr;
    }
    if (offsets[0] != 0) {
        set_error("carma_mctx_create: offsets[0] must be 0 (got %ld)", offsets[0]);
        return nullptr;
    }
    for (int s = 0; s < nseries; s++) {
        if (offsets[s + 1] < offsets[s]) {
            set_error("carma_mctx_create: offsets must be non-decreasing (offsets[%d]=%ld > offsets[%d]=%ld)", s, offsets[s], s + 1,
                      offsets[s + 1]);
            return nullptr;
        }
        if (offsets[s + 1] - offsets[s] > 0x7fffffffL - P3L_PAD_RECORDS) {
            set_error("carma_mctx_create: series %d is longer than an int can count", s);
            return nullptr;
        }
    }
    // every series prepared as carma_ctx_create prepares one (host only: all argument errors come before any device work)
    Mctx* c = new Mctx();
    c->device = device;
    c->p = p;
    c->q = q;
    c->d = (p == 1) ? 4 : 3 + p + q;
    c->S = nseries;
    c->hoff.assign(nseries + 1, 0);
    c->off.resize(nseries);
    c->n.resize(nseries);
    c->pr.resize(nseries);
    c->repdt.resize(nseries);
    std::vector<std::vector<double>> packed(nseries);
    long rec_total = 0;
    for (int s = 0; s < nseries; s++) {
        const long a = offsets[s], b = offsets[s + 1];
        std::vector<double> ts(time + a, time + b), ys(y + a, y + b), es(yerr + a, yerr + b);
        sort_dedup(ts, ys, es);
        const long ns = (long)ts.size();
        if (ns < 2) {
            set_error("carma_mctx_create: series %d has fewer than 2 distinct times", s);
            delete c;
            return nullptr;
        }
        double ms = 0.0;
        if (max_stdev) {
            ms = max_stdev[s];
        } else {                                              // 10 sqrt(var(y, ddof=1)) of the series as given (Context's default)
            double mean = 0.0, ss = 0.0;
            for (long k = a; k < b; k++) mean += y[k];
            mean /= (double)(b - a);
            for (long k = a; k < b; k++) ss += (y[k] - mean) * (y[k] - mean);
            ms = 10.0 * std::sqrt(ss / (double)(b - a - 1));
        }
        c->pr[s].measerr_dof = 50.0;   // src/include/carpack.hpp:63
        set_prior_bounds(c->pr[s], ts.data(), ns, ms);
        packed[s] = pack_series(ts, ys, es);
        c->repdt[s] = series_repeated_dt(packed[s].data(), ns);
        c->n[s] = (int)ns;
        c->off[s] = rec_total;
        rec_total += (ns + P3L_PAD_RECORDS + 1) / 2 * 2;     // records and pad records, the next series on a 64-byte boundary
        c->hoff[s + 1] = c->hoff[s] + ns;
        c->t.insert(c->t.end(), ts.begin(), ts.end());
        c->y.insert(c->y.end(), ys.begin(), ys.end());
        c->yerr.insert(c->yerr.end(), es.begin(), es.end());
    }
    if (select_device(device) != CARMA_OK) {
        delete c;
        return nullptr;
    }
    std::vector<double> rec((size_t)rec_total * 4, 0.0);
    for (int s = 0; s < nseries; s++) {
        const size_t nr = (size_t)c->n[s] + P3L_PAD_RECORDS;         // the records and pads of pack_series (its tail arrays stay out)
        std::memcpy(&rec[(size_t)c->off[s] * 4], packed[s].data(), sizeof(double) * 4 * nr);
        std::vector<double>().swap(packed[s]);
    }
    hipError_t e = c->d_rec.alloc(sizeof(double) * rec.size());
    if (e == hipSuccess) e = hipMemcpy(c->d_rec.as<void>(), rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = c->d_off.alloc(sizeof(long) * nseries);
    if (e == hipSuccess) e = hipMemcpy(c->d_off.as<void>(), c->off.data(), sizeof(long) * nseries, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = c->d_n.alloc(sizeof(int) * nseries);
    if (e == hipSuccess) e = hipMemcpy(c->d_n.as<void>(), c->n.data(), sizeof(int) * nseries, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = c->d_pr.alloc(sizeof(Prior) * nseries);
    if (e == hipSuccess) e = hipMemcpy(c->d_pr.as<void>(), c->pr.data(), sizeof(Prior) * nseries, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        hip_fail(e, "carma_mctx_create");
        carma_mctx_destroy(reinterpret_cast<carma_mctx*>(c));
        return nullptr;
    }
    return reinterpret_cast<carma_mctx*>(c);
}

void carma_mctx_destroy(carma_mctx* h)
{
    if (!h) return;
    Mctx* c = reinterpret_cast<Mctx*>(h);
    (void)hipSetDevice(c->device);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    mpt_free(c);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;                                                 // (the DevMem members release their buffers)
}

int carma_mctx_nseries(const carma_mctx* h) { return h ? reinterpret_cast<const Mctx*>(h)->S : CARMA_EINVAL; }
int carma_mctx_dim(const carma_mctx* h) { return h ? reinterpret_cast<const Mctx*>(h)->d : CARMA_EINVAL; }

int carma_mctx_n(const carma_mctx* h, int s)
{
    if (!h || s < 0 || s >= reinterpret_cast<const Mctx*>(h)->S) return CARMA_EINVAL;
    return reinterpret_cast<const Mctx*>(h)->n[s];
}

int carma_mctx_get_data(const carma_mctx* h, int s, double* time, double* y, double* yerr)
{
    if (!h || s < 0 || s >= reinterpret_cast<const Mctx*>(h)->S) return CARMA_EINVAL;
    const Mctx* c = reinterpret_cast<const Mctx*>(h);
    const size_t a = (size_t)c->hoff[s], n = (size_t)c->n[s];
    if (time) std::memcpy(time, c->t.data() + a, sizeof(double) * n);
    if (y) std::memcpy(y, c->y.data() + a, sizeof(double) * n);
    if (yerr) std::memcpy(yerr, c->yerr.data() + a, sizeof(double) * n);
    return CARMA_OK;
}

int carma_mctx_get_prior(const carma_mctx* h, int s, double* out3)
{
    if (!h || !out3 || s < 0 || s >= reinterpret_cast<const Mctx*>(h)->S) return CARMA_EINVAL;
    const Prior& pr = reinterpret_cast<const Mctx*>(h)->pr[s];
    out3[0] = pr.max_stdev;
    out3[1] = pr.max_freq;
    out3[2] = pr.min_freq;
    return CARMA_OK;
}

int carma_mlogdensity_batch(carma_mctx* h, const double* theta, const int* series, int B, int ignore_prior, double* out)
{
    if (!h || B < 0 || (B > 0 && (!theta || !series || !out))) {
        set_error("carma_mlogdensity_batch: bad argument");
        return CARMA_EINVAL;
    }
    if (B == 0) return CARMA_OK;
    Mctx* c = reinterpret_cast<Mctx*>(h);
    const int S = c->S, d = c->d;
    // launch plan (host, O(B + S log S)): counting sort of the evaluations by series, waves of 64 per series, longest
    // series first, the regular-cadence series (REPDT) in a launch of their own
    c->cnt.assign(S, 0);
    for (int i = 0; i < B; i++) {
        const int s = series[i];
        if (s < 0 || s >= S) {
            set_error("carma_mlogdensity_batch: series[%d] = %d out of range (nseries = %d)", i, s, S);
            return CARMA_EINVAL;
        }
        c->cnt[s]++;
    }
    c->first.assign(S + 1, 0);
    for (int s = 0; s < S; s++) c->first[s + 1] = c->first[s] + c->cnt[s];
    c->order.resize(B);
    {
        std::vector<int>& pos = c->wser_tmp;
        pos.assign(c->first.begin(), c->first.end() - 1);
        for (int i = 0; i < B; i++) c->order[pos[series[i]]++] = i;
    }
    std::vector<int> used;
    used.reserve(S);
    long W = 0;
    for (int s = 0; s < S; s++)
        if (c->cnt[s]) {
            used.push_back(s);
            W += (c->cnt[s] + 63) / 64;
        }
    std::stable_sort(used.begin(), used.end(), [&](int a, int b) {
        if (c->repdt[a] != c->repdt[b]) return c->repdt[a] < c->repdt[b];
        return c->n[a] > c->n[b];
    });
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    int rc = c->ensure(B, W);
    if (rc != CARMA_OK) return rc;
    double* h_th = reinterpret_cast<double*>(c->h_stage);
    double* h_out = h_th + (size_t)c->cap_B * d;
    int* h_wser = reinterpret_cast<int*>(h_out + c->cap_B);
    int* h_eidx = h_wser + c->cap_W;
    std::memcpy(h_th, theta, sizeof(double) * (size_t)B * d);
    long w = 0, w_plain = 0;                                  // waves of the REPDT = false launch: the first w_plain
    for (int s : used) {
        if (!c->repdt[s]) w_plain += (c->cnt[s] + 63) / 64;
        for (int k = c->first[s]; k < c->first[s + 1]; k += 64, w++) {
            h_wser[w] = s;
            int* ew = h_eidx + (size_t)w * 64;
            const int m = std::min(64, c->first[s + 1] - k);
            std::memcpy(ew, &c->order[k], sizeof(int) * m);
            for (int l = m; l < 64; l++) ew[l] = -1;
        }
    }
    hipStream_t st = c->stream;
    double *d_theta = c->d_theta.as<double>(), *d_out = c->d_out.as<double>();
    int *d_wser = c->d_wser.as<int>(), *d_eidx = c->d_eidx.as<int>();
    e = hipMemcpyAsync(d_theta, h_th, sizeof(double) * (size_t)B * d, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_wser, h_wser, sizeof(int) * (size_t)W, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_eidx, h_eidx, sizeof(int) * (size_t)W * 64, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return hip_fail(e, "carma_mlogdensity_batch: H2D");
    (void)hipGetLastError();   // HIP's last-error is sticky: drop anything left by earlier calls
    e = launch_logdens_ms(c->p, false, d_theta, d, c->q, c->rec(), c->offs(), c->ns(), c->prs(), d_wser, d_eidx, w_plain, ignore_prior,
                          d_out, st);
    if (e == hipSuccess)
        e = launch_logdens_ms(c->p, true, d_theta, d, c->q, c->rec(), c->offs(), c->ns(), c->prs(), d_wser + w_plain,
                              d_eidx + (size_t)w_plain * 64, W - w_plain, ignore_prior, d_out, st);
    if (e != hipSuccess) return hip_fail(e, "carma_mlogdensity_batch: launch");
    e = hipMemcpyAsync(h_out, d_out, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, "carma_mlogdensity_batch: D2H");
    std::memcpy(out, h_out, sizeof(double) * (size_t)B);
    return CARMA_OK;
}

int carma_mkfilter(carma_mctx* h, const int* series, int M, const double* sigsqr, const double* omega_re_im, const double* ma,
                   int nma, const double* mu, double* mean, double* var, long* out_offsets, int* singular)
{
    if (!h || !mean || !var) {
        set_error("carma_mkfilter: bad argument (null context or output)");
        return CARMA_EINVAL;
    }
    Mctx* c = reinterpret_cast<Mctx*>(h);
    const int p = c->p, PW = p == 1 ? 3 : 3 * p + 2;
    std::vector<double> par;
    int rc = pack_items(c, "carma_mkfilter", series, M, sigsqr, omega_re_im, ma, nma, mu, par);
    if (rc != CARMA_OK) return rc;
    // launch plan (host): the items sorted by length, longest first -- slot j is lane j % 64 of wave j / 64, and the lanes of
    // a wave run to the wave's longest series
    std::vector<long> offs((size_t)M + 1, 0);
    for (int i = 0; i < M; i++) offs[i + 1] = offs[i] + c->n[series[i]];
    const long total = offs[M];
    std::vector<int>& order = c->order;
    order.resize(M);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return c->n[series[a]] > c->n[series[b]]; });
    const long W = ((long)M + 63) / 64;
    std::vector<double> spar((size_t)M * PW);
    std::vector<int> tint((size_t)2 * M);                     // slot_series [M], slot_n [M]
    std::vector<long> tlong((size_t)W + M);                   // tile_off [W], slot_out [M]
    size_t tile_total = 0;
    for (long j = 0; j < M; j++) {
        const int i = order[j], sidx = series[i];
        std::memcpy(&spar[(size_t)j * PW], &par[(size_t)i * PW], sizeof(double) * PW);
        tint[j] = sidx;
        tint[(size_t)M + j] = c->n[sidx];
        tlong[(size_t)W + j] = offs[i];
        if (j % 64 == 0) {
            tlong[j / 64] = (long)tile_total;
            tile_total += (size_t)2 * c->n[sidx] * (size_t)std::min(64L, (long)M - j);
        }
    }
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    hipStream_t st = c->stream;
    std::vector<int> sing((size_t)M, 0);
    e = upload(c->k_par, spar, st);
    if (e == hipSuccess) e = upload(c->k_int, tint, st);
    if (e == hipSuccess) e = upload(c->k_long, tlong, st);
    if (e == hipSuccess) e = c->k_tile.need(sizeof(double) * tile_total);
    if (e == hipSuccess) e = c->k_res.need(sizeof(double) * 2 * (size_t)total);
    if (e == hipSuccess) e = c->k_sing.need(sizeof(int) * (size_t)M);
    if (e == hipSuccess) {
        (void)hipGetLastError();   // HIP's last-error is sticky: drop anything left by earlier calls
        const double* d_par = c->k_par.as<double>();
        const int *d_sser = c->k_int.as<int>(), *d_sn = d_sser + M;
        const long *d_toff = c->k_long.as<long>(), *d_sout = d_toff + W;
        double *d_mv = c->k_tile.as<double>(), *d_mean = c->k_res.as<double>(), *d_var = d_mean + total;
        const dim3 grid((unsigned)W), block(64);
        switch (p) {
            case 1:
                hipLaunchKernelGGL(k_mkfilter_car1, grid, block, 0, st, d_par, M, c->rec(), c->offs(), c->ns(), d_sser, d_toff, d_mv);
                break;
#define CARMA_MKF(N)                                                                                                              \
    case N:                                                                                                                       \
        hipLaunchKernelGGL((k_mkfilter_carma_lane<N>), grid, block, 0, st, d_par, M, c->rec(), c->offs(), c->ns(), d_sser,        \
                           d_toff, d_mv, c->k_sing.as<int>());                                                                    \
        break;
                CARMA_MKF(2) CARMA_MKF(3) CARMA_MKF(4) CARMA_MKF(5) CARMA_MKF(6) CARMA_MKF(7)
#undef CARMA_MKF
            default: return CARMA_EINVAL;
        }
        e = hipGetLastError();
        if (e == hipSuccess) {
            const long nmax = c->n[series[order[0]]];
            const dim3 tgrid((unsigned)W, (unsigned)std::min((nmax + 31) / 32, 1024L));
            hipLaunchKernelGGL(k_mtranspose_mv, tgrid, dim3(256), 0, st, d_mv, d_toff, M, d_sn, d_sout, d_mean, d_var);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(mean, d_mean, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(var, d_var, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && p > 1)
            e = hipMemcpyAsync(sing.data(), c->k_sing.as<int>(), sizeof(int) * (size_t)M, hipMemcpyDeviceToHost, st);
    }
    const hipError_t es = hipStreamSynchronize(st);           // (also after a failure: enqueued copies read and write this frame's vectors)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return hip_fail(e, "carma_mkfilter");
    if (out_offsets) std::memcpy(out_offsets, offs.data(), sizeof(long) * ((size_t)M + 1));
    if (singular)
        for (long j = 0; j < M; j++) singular[order[j]] = sing[j];
    return CARMA_OK;
}

int carma_mpredict(carma_mctx* h, const int* series, int M, const double* sigsqr, const double* omega_re_im, const double* ma,
                   int nma, const double* mu, const double* tpred, const long* toff, double* pmean, double* pvar, int* singular)
{
    if (!h || !toff) {
        set_error("carma_mpredict: bad argument (null context or toff)");
        return CARMA_EINVAL;
    }
    Mctx* c = reinterpret_cast<Mctx*>(h);
    const int p = c->p;
    std::vector<double> par;
    int rc = pack_items(c, "carma_mpredict", series, M, sigsqr, omega_re_im, ma, nma, mu, par);
    if (rc != CARMA_OK) return rc;
    if (toff[0] < 0) {
        set_error("carma_mpredict: toff[0] = %ld is negative", toff[0]);
        return CARMA_EINVAL;
    }
    for (int i = 0; i < M; i++)
        if (toff[i + 1] < toff[i]) {
            set_error("carma_mpredict: item %d: toff must be non-decreasing (toff[%d]=%ld > toff[%d]=%ld)", i, i, toff[i], i + 1,
                      toff[i + 1]);
            return CARMA_EINVAL;
        }
    const long t0 = toff[0], T = toff[M] - t0;
    if (T > 0 && (!tpred || !pmean || !pvar)) {
        set_error("carma_mpredict: bad argument (null tpred, pmean or pvar)");
        return CARMA_EINVAL;
    }
    if (singular) std::fill(singular, singular + M, 0);
    if (T == 0) return CARMA_OK;
    // launch plan (host).  p = 1: a lane per (item, time) pair in the caller's order.  p >= 2: the pairs grouped by series
    // (counting sort of the items), 64 / G of them per wave, a wave on one series, the longest series first.
    std::vector<int> tint;
    std::vector<long> tlong;
    long W = 0;
    const int E = p == 1 ? 64 : 64 / group_of(p);
    if (p == 1) {
        tint.resize((size_t)M + T);                           // item_series [M], pair_item [T]
        for (int i = 0; i < M; i++) {
            tint[i] = series[i];
            std::fill(tint.begin() + M + (toff[i] - t0), tint.begin() + M + (toff[i + 1] - t0), i);
        }
        W = (T + 63) / 64;
    } else {
        const int S = c->S;
        std::vector<long> npair((size_t)S, 0);
        c->cnt.assign(S, 0);
        for (int i = 0; i < M; i++) {
            c->cnt[series[i]]++;
            npair[series[i]] += toff[i + 1] - toff[i];
        }
        c->first.assign(S + 1, 0);
        for (int s = 0; s < S; s++) c->first[s + 1] = c->first[s] + c->cnt[s];
        c->order.resize(M);
        {
            std::vector<int>& pos = c->wser_tmp;
            pos.assign(c->first.begin(), c->first.end() - 1);
            for (int i = 0; i < M; i++) c->order[pos[series[i]]++] = i;
        }
        std::vector<int> used;
        for (int s = 0; s < S; s++)
            if (npair[s]) {
                used.push_back(s);
                W += (npair[s] + E - 1) / E;
            }
        std::stable_sort(used.begin(), used.end(), [&](int a, int b) { return c->n[a] > c->n[b]; });
        tint.assign((size_t)W + (size_t)W * E, 0);            // wave_series [W], pair_item [W E]
        tlong.assign((size_t)W * E, -1L);                     // pair_out [W E]
        long w = 0;
        for (int s : used) {
            long g = w * E;                                   // next group of this series
            for (int k = c->first[s]; k < c->first[s + 1]; k++) {
                const int i = c->order[k];
                for (long o = toff[i] - t0; o < toff[i + 1] - t0; o++, g++) {
                    tint[(size_t)W + g] = i;
                    tlong[g] = o;
                }
            }
            const long w1 = w + (npair[s] + E - 1) / E;
            for (; w < w1; w++) tint[w] = s;
        }
    }
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    hipStream_t st = c->stream;
    std::vector<int> sing((size_t)M, 0);
    const size_t npar = par.size();
    e = c->k_par.need(sizeof(double) * (npar + (size_t)T));
    if (e == hipSuccess) e = hipMemcpyAsync(c->k_par.as<void>(), par.data(), sizeof(double) * npar, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->k_par.as<double>() + npar, tpred + t0, sizeof(double) * (size_t)T, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = upload(c->k_int, tint, st);
    if (e == hipSuccess && p > 1) e = upload(c->k_long, tlong, st);
    if (e == hipSuccess) e = c->k_res.need(sizeof(double) * 2 * (size_t)T);
    if (e == hipSuccess) e = c->k_sing.need(sizeof(int) * (size_t)M);
    if (e == hipSuccess) e = hipMemsetAsync(c->k_sing.as<int>(), 0, sizeof(int) * (size_t)M, st);
    if (e == hipSuccess) {
        (void)hipGetLastError();
        const double *d_par = c->k_par.as<double>(), *d_tp = d_par + npar;
        double *d_pm = c->k_res.as<double>(), *d_pv = d_pm + T;
        const int* d_int = c->k_int.as<int>();
        const dim3 grid((unsigned)W), block(64);
        switch (p) {
            case 1:
                hipLaunchKernelGGL(k_mpredict_car1, grid, block, 0, st, d_par, c->rec(), c->offs(), c->ns(), d_int, d_int + M, T, d_tp,
                                   d_pm, d_pv);
                break;
#define CARMA_MPR(N)                                                                                                              \
    case N:                                                                                                                       \
        hipLaunchKernelGGL((k_mpredict_carma<N, GroupOf<N>::value>), grid, block, 0, st, d_par, c->rec(), c->offs(), c->ns(),     \
                           d_int, d_int + W, c->k_long.as<long>(), d_tp, d_pm, d_pv, c->k_sing.as<int>());                        \
        break;
                CARMA_MPR(2) CARMA_MPR(3) CARMA_MPR(4) CARMA_MPR(5) CARMA_MPR(6) CARMA_MPR(7)
#undef CARMA_MPR
            default: return CARMA_EINVAL;
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(pmean + t0, d_pm, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(pvar + t0, d_pv, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(sing.data(), c->k_sing.as<int>(), sizeof(int) * (size_t)M, hipMemcpyDeviceToHost, st);
    }
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return hip_fail(e, "carma_mpredict");
    if (singular) std::memcpy(singular, sing.data(), sizeof(int) * (size_t)M);
    return CARMA_OK;
}

int carma_msmooth(carma_mctx* h, const int* series, int M, const double* sigsqr, const double* omega_re_im, const double* ma,
                  int nma, const double* mu, const double* tout, const long* toff, double* mean, double* var, int* singular)
{
    static const char* const who = "carma_msmooth";
    if (!h || !toff) {
        set_error("%s: bad argument (null context or toff)", who);
        return CARMA_EINVAL;
    }
    Mctx* c = reinterpret_cast<Mctx*>(h);
    const int p = c->p;
    std::vector<double> par;
    int rc = pack_items(c, who, series, M, sigsqr, omega_re_im, ma, nma, mu, par);
    if (rc != CARMA_OK) return rc;
    if (toff[0] < 0) {
        set_error("%s: toff[0] = %ld is negative", who, toff[0]);
        return CARMA_EINVAL;
    }
    for (int i = 0; i < M; i++)
        if (toff[i + 1] < toff[i]) {
            set_error("%s: item %d: toff must be non-decreasing (toff[%d]=%ld > toff[%d]=%ld)", who, i, i, toff[i], i + 1, toff[i + 1]);
            return CARMA_EINVAL;
        }
    const long t0 = toff[0], T = toff[M] - t0;
    if (T > 0 && (!tout || !mean || !var)) {
        set_error("%s: bad argument (null tout, mean or var)", who);
        return CARMA_EINVAL;
    }
    for (int i = 0; i < M; i++)
        for (long o = toff[i]; o < toff[i + 1]; o++)
            if (!std::isfinite(tout[o])) {
                set_error("%s: item %d: tout[%ld] is not finite", who, i, o);
                return CARMA_EINVAL;
            }
    if (singular) std::fill(singular, singular + M, 0);
    if (T == 0) return CARMA_OK;
    // launch plan (host): the items with times sorted by (series, time list); a run of equal keys is a job
    const int G = p > 1 ? group_of(p) : 0, E = G ? 64 / G : 64;
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
    std::vector<double> grids;
    for (size_t k = 0; k < ord.size();) {
        size_t k1 = k + 1;
        while (k1 < ord.size() && cmp(ord[k], ord[k1]) == 0) k1++;
        const int i0 = ord[k], s = series[i0], job = (int)job_series.size();
        const SmoothGrid sg = smooth_merge(c->t.data() + c->hoff[s], c->n[s], tout + toff[i0], (int)len(i0));
        job_series.push_back(s);
        job_ng.push_back(sg.ng);
        job_goff.push_back((long)grids.size());
        grids.insert(grids.end(), sg.grid.begin(), sg.grid.end());
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
    const long W = (long)wave_job.size(), J = (long)job_series.size();
    // chunks of consecutive waves under the scratch cap ("SMOOTH_CHUNK_MODELS": that many models' waves); wave_pts: grid points
    // of the waves before w in its chunk
    const long forced = tune_get(TUNE_SMOOTH_CHUNK_MODELS);
    const long wmax = (forced != TUNE_UNSET && forced > 0) ? (forced + E - 1) / E : W;
    std::vector<long> wave_pts((size_t)W), chunk0;
    size_t pts_max = 0;
    {
        size_t pts = 0;
        long nw = 0;
        for (long w = 0; w < W; w++) {
            const size_t ng = (size_t)job_ng[wave_job[w]];
            if (w == 0 || nw >= wmax || smooth_wave_bytes(G, 1) * (pts + ng) > SMOOTH_SCRATCH_CAP) {
                chunk0.push_back(w);
                pts = 0;
                nw = 0;
            }
            wave_pts[w] = (long)pts;
            pts += ng;
            nw++;
            pts_max = std::max(pts_max, pts);
        }
        chunk0.push_back(W);
    }
    // tables: ints [wave_job W][job_series J][job_ng J][slot_item W E][src], longs [job_goff J][slot_out W E][wave_pts W]
    std::vector<int> tint;
    tint.insert(tint.end(), wave_job.begin(), wave_job.end());
    tint.insert(tint.end(), job_series.begin(), job_series.end());
    tint.insert(tint.end(), job_ng.begin(), job_ng.end());
    tint.insert(tint.end(), slot_item.begin(), slot_item.end());
    tint.insert(tint.end(), srcs.begin(), srcs.end());
    std::vector<long> tlong;
    tlong.insert(tlong.end(), job_goff.begin(), job_goff.end());
    tlong.insert(tlong.end(), slot_out.begin(), slot_out.end());
    tlong.insert(tlong.end(), wave_pts.begin(), wave_pts.end());
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    hipStream_t st = c->stream;
    std::vector<int> sing((size_t)M, 0);
    const size_t npar = par.size();
    e = c->k_par.need(sizeof(double) * (npar + grids.size()));
    if (e == hipSuccess) e = hipMemcpyAsync(c->k_par.as<void>(), par.data(), sizeof(double) * npar, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c->k_par.as<double>() + npar, grids.data(), sizeof(double) * grids.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = upload(c->k_int, tint, st);
    if (e == hipSuccess) e = upload(c->k_long, tlong, st);
    if (e == hipSuccess) e = c->k_tile.need(smooth_wave_bytes(G, 1) * pts_max);
    if (e == hipSuccess) e = c->k_res.need(sizeof(double) * 2 * (size_t)T);
    if (e == hipSuccess) e = c->k_sing.need(sizeof(int) * (size_t)M);
    if (e == hipSuccess) e = hipMemsetAsync(c->k_sing.as<int>(), 0, sizeof(int) * (size_t)M, st);
    if (e == hipSuccess) {
        (void)hipGetLastError();
        const double* d_par = c->k_par.as<double>();
        const int* di = c->k_int.as<int>();
        const long* dl = c->k_long.as<long>();
        MsmoothTabs tb;
        tb.wave_job = di;
        tb.job_series = di + W;
        tb.job_ng = tb.job_series + J;
        tb.slot_item = tb.job_ng + J;
        tb.src = tb.slot_item + W * E;
        tb.job_goff = dl;
        tb.slot_out = dl + J;
        tb.wave_pts = tb.slot_out + W * E;
        tb.grid = d_par + npar;
        double *d_m = c->k_res.as<double>(), *d_v = d_m + T;
        // a chunk's scratch: the lane records of its waves, then their group records
        double4* rec = c->k_tile.as<double4>();
        double4* grp = rec + pts_max * 64;
        for (size_t ci = 0; ci + 1 < chunk0.size() && e == hipSuccess; ci++) {
            const long w0 = chunk0[ci];
            const dim3 grid((unsigned)(chunk0[ci + 1] - w0)), block(64);
            switch (p) {
                case 1:
                    hipLaunchKernelGGL(k_msmooth_car1, grid, block, 0, st, d_par, c->rec(), c->offs(), tb, w0, c->k_tile.as<double>(),
                                       d_m, d_v);
                    break;
#define CARMA_MSM(N)                                                                                                              \
    case N:                                                                                                                       \
        hipLaunchKernelGGL((k_msmooth_carma<N, GroupOf<N>::value>), grid, block, 0, st, d_par, c->rec(), c->offs(), tb, w0, rec,   \
                           grp, d_m, d_v, c->k_sing.as<int>());                                                                   \
        break;
                    CARMA_MSM(2) CARMA_MSM(3) CARMA_MSM(4) CARMA_MSM(5) CARMA_MSM(6) CARMA_MSM(7)
#undef CARMA_MSM
                default: return CARMA_EINVAL;
            }
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(mean + t0, d_m, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(var + t0, d_v, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(sing.data(), c->k_sing.as<int>(), sizeof(int) * (size_t)M, hipMemcpyDeviceToHost, st);
    }
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return hip_fail(e, who);
    if (singular) std::memcpy(singular, sing.data(), sizeof(int) * (size_t)M);
    return CARMA_OK;
}

int carma_mlogdensity_kernel_name(const carma_mctx* h, char* buf, int len)
{
    if (!h || !buf || len < 1) return CARMA_EINVAL;
    const Mctx* c = reinterpret_cast<const Mctx*>(h);
    const int r = c->p == 1 ? snprintf(buf, len, "k_logdens_car1_ms") : snprintf(buf, len, "k_logdens_carma_lane_ms<%d>", c->p);
    return r > 0 ? CARMA_OK : CARMA_EINVAL;
}

// ---- carma_mpt_*: the parallel-tempering sampler over many series -------------------------------------------------------

int carma_mpt_create(carma_mctx* h, const int* series, int M, int ntemps, int nreplicas, const double* temperatures, int adapt_iters,
                     uint64_t seed)
{
    if (!h || !series || nreplicas < 1 || adapt_iters < 0) {
        set_error("carma_mpt_create: bad argument (null context or series, nreplicas < 1 or adapt_iters < 0)");
        return CARMA_EINVAL;
    }
    if (M < 1) {
        set_error("carma_mpt_create: need at least one run (got M = %d)", M);
        return CARMA_EINVAL;
    }
    if (ntemps < 1 || ntemps > 64) {
        set_error("carma_mpt_create: a ladder is 1 ... 64 temperatures, the lanes of a wave (got %d)", ntemps);
        return CARMA_EINVAL;
    }
    Mctx* c = reinterpret_cast<Mctx*>(h);
    for (int j = 0; j < M; j++)
        if (series[j] < 0 || series[j] >= c->S) {
            set_error("carma_mpt_create: run %d: series index %d out of range (nseries = %d)", j, series[j], c->S);
            return CARMA_EINVAL;
        }
    // (chain and ladder indices are ints in the launch arguments, evaluation counts in carma_mlogdensity_batch too)
    const long long nc_ll = (long long)M * nreplicas * ntemps;
    if (nc_ll > 0x7fffffffLL - 64) {
        set_error("carma_mpt_create: %d runs x %d replicas x %d temperatures = %lld chains, more than one launch can index (%lld)", M,
                  nreplicas, ntemps, nc_ll, 0x7fffffffLL - 64);
        return CARMA_EINVAL;
    }
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    mpt_free(c);
    MptState* s = new MptState();
    c->mpt = s;
    s->M = M;
    s->reps = nreplicas;
    s->maxiter = adapt_iters;
    s->seed = seed;
    s->series.assign(series, series + M);
    std::vector<double> temps;
    default_ladder(ntemps, temperatures, temps);             // shared by all runs
    const int d = c->d, nlad = M * nreplicas;
    const size_t nchain = (size_t)nc_ll;
    // initial proposal factor of run j, from ITS series
    std::vector<double> chol(nchain * d * d, 0.0), R0((size_t)d * d);
    std::vector<int> lser((size_t)nlad);
    for (int j = 0; j < M; j++) {
        const int sj = series[j];
        const long n = c->n[sj];
        s->nmax = std::max(s->nmax, (int)n);
        (c->repdt[sj] ? s->any_rep : s->any_plain) = true;
        initial_factor(pop_var(c->y.data() + c->hoff[sj], n), n, d, R0.data());
        for (size_t k = (size_t)j * nreplicas * ntemps; k < (size_t)(j + 1) * nreplicas * ntemps; k++)
            std::memcpy(&chol[k * d * d], R0.data(), sizeof(double) * d * d);
        for (int r = 0; r < nreplicas; r++) lser[(size_t)j * nreplicas + r] = sj;
    }
    e = pt_ens_create(s, ntemps, nlad, d, temps, chol.data());
    if (e == hipSuccess) e = dev_malloc(&s->d_lser, sizeof(int) * lser.size());
    if (e == hipSuccess) e = dev_malloc(&s->d_rep, sizeof(char) * (size_t)c->S);
    if (e == hipSuccess) e = dev_malloc(&s->d_scratch, sizeof(double) * pt_lane_scratch_doubles(d, (long)nchain));
    if (e == hipSuccess) e = hipMemcpy(s->d_lser, lser.data(), sizeof(int) * lser.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_rep, c->repdt.data(), sizeof(char) * (size_t)c->S, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        const int rc = hip_fail(e, "carma_mpt_create");
        mpt_free(c);
        return rc;
    }
    return CARMA_OK;
}

int carma_mpt_set_chains(carma_mctx* h, const double* theta, const double* logpost)
{
    MptState* s = mpt_state(h, "carma_mpt_set_chains", false);
    if (!s) return CARMA_EINVAL;
    if (!theta) {
        set_error("carma_mpt_set_chains: null theta");
        return CARMA_EINVAL;
    }
    Mctx* c = reinterpret_cast<Mctx*>(h);
    const size_t nchain = s->nchain();
    std::vector<double> lp(nchain);
    if (logpost) {
        std::memcpy(lp.data(), logpost, sizeof(double) * nchain);
    } else {
        std::vector<int> which(nchain);
        for (size_t k = 0; k < nchain; k++) which[k] = s->series[k / ((size_t)s->reps * s->T)];
        const int rc = carma_mlogdensity_batch(h, theta, which.data(), (int)nchain, 0, lp.data());
        if (rc != CARMA_OK) return rc;
    }
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = pt_ens_set_chains(s, c->d, theta, lp.data());
    if (e != hipSuccess) return hip_fail(e, "carma_mpt_set_chains");
    s->started = true;
    return CARMA_OK;
}

int carma_mpt_get_chains(carma_mctx* h, double* theta, double* logpost)
{
    MptState* s = mpt_state(h, "carma_mpt_get_chains", false);
    if (!s) return CARMA_EINVAL;
    Mctx* c = reinterpret_cast<Mctx*>(h);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = pt_ens_get_chains(s, c->d, theta, logpost);
    if (e != hipSuccess) return hip_fail(e, "carma_mpt_get_chains");
    return CARMA_OK;
}

int carma_mpt_start(carma_mctx* h, const double* init)
{
    MptState* s = mpt_state(h, "carma_mpt_start", false);
    if (!s) return CARMA_EINVAL;
    Mctx* c = reinterpret_cast<Mctx*>(h);
    const int d = c->d, M = s->M;
    const size_t per_run = (size_t)s->reps * s->T, nchain = s->nchain();
    std::vector<double> theta(nchain * d), lp(nchain, -std::numeric_limits<double>::infinity());
    std::vector<char> done(nchain, 0);
    // a run's init row is honoured when its log-density on the run's series is finite (src/samplers.cpp:75-93): all M rows in one
    // launch
    if (init) {
        std::vector<double> l0(M);
        const int rc = carma_mlogdensity_batch(h, init, s->series.data(), M, 0, l0.data());
        if (rc != CARMA_OK) return rc;
        for (int j = 0; j < M; j++) {
            if (!std::isfinite(l0[j])) continue;
            for (size_t k = j * per_run; k < (j + 1) * per_run; k++) {
                std::memcpy(&theta[k * d], init + (size_t)j * d, sizeof(double) * d);
                lp[k] = l0[j];
                done[k] = 1;
            }
        }
    }
    // Drawn starts: chain k = ladder T + temperature of the ENSEMBLE keys its generator, so run j draws what a single-series sampler
    // sharded to replica0 = j R draws; the candidates still pending of ALL runs are evaluated in one launch per round.
    std::vector<int> which;
    const int rc = find_starts(
        nchain, d, theta.data(), lp.data(), done.data(),
        [&](size_t k, int round, double* out) {
            const int sj = s->series[k / per_run];
            std::mt19937_64 rng = start_rng(s->seed, (uint64_t)k, round);
            draw_start(c->t.data() + c->hoff[sj], c->y.data() + c->hoff[sj], c->n[sj], c->pr[sj], c->p, c->q, rng, out);
        },
        [&](const double* cand, const size_t* idx, size_t m, double* out) {
            which.resize(m);
            for (size_t i = 0; i < m; i++) which[i] = s->series[idx[i] / per_run];
            return carma_mlogdensity_batch(h, cand, which.data(), (int)m, 0, out);
        });
    if (rc != CARMA_OK) return rc;
    for (size_t k = 0; k < nchain; k++)
        if (!done[k]) {
            set_error("carma_mpt_start: no finite starting value found for chain %zu of run %zu (series %d)", k % per_run, k / per_run,
                      s->series[k / per_run]);
            return CARMA_EINVAL;
        }
    return carma_mpt_set_chains(h, theta.data(), lp.data());
}

int carma_mpt_get_factor(carma_mctx* h, double* chol)
{
    MptState* s = mpt_state(h, "carma_mpt_get_factor", false);
    if (!s || !chol) return CARMA_EINVAL;
    Mctx* c = reinterpret_cast<Mctx*>(h);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = pt_ens_get_factor(s, c->d, c->stream, chol);
    if (e != hipSuccess) return hip_fail(e, "carma_mpt_get_factor");
    return CARMA_OK;
}

int carma_mpt_set_factor(carma_mctx* h, const double* chol)
{
    MptState* s = mpt_state(h, "carma_mpt_set_factor", false);
    if (!s || !chol) return CARMA_EINVAL;
    Mctx* c = reinterpret_cast<Mctx*>(h);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = pt_ens_set_factor(s, c->d, c->stream, chol);
    if (e != hipSuccess) return hip_fail(e, "carma_mpt_set_factor");
    return CARMA_OK;
}

int carma_mpt_iterate(carma_mctx* h, long niter, int do_exchange)
{
    MptState* s = mpt_state(h, "carma_mpt_iterate", true);
    if (!s) return CARMA_EINVAL;
    if (niter < 0) {
        set_error("carma_mpt_iterate: niter < 0");
        return CARMA_EINVAL;
    }
    Mctx* c = reinterpret_cast<Mctx*>(h);
    const hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    return mpt_iterate(c, niter, do_exchange, 0, nullptr);
}

int carma_mpt_sample(carma_mctx* h, int nsamples, int thin, double* samples, double* logposts)
{
    MptState* s = mpt_state(h, "carma_mpt_sample", true);
    if (!s) return CARMA_EINVAL;
    if (nsamples < 1 || thin < 1 || !samples || !logposts) {
        set_error("carma_mpt_sample: bad argument (nsamples >= 1, thin >= 1, non-null outputs)");
        return CARMA_EINVAL;
    }
    Mctx* c = reinterpret_cast<Mctx*>(h);
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    long capacity = 0;
    e = pt_ens_reserve_samples(s, c->d, nsamples, &capacity);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("carma_mpt_sample: no device memory for the sample buffer: %zu bytes asked for (%ld ladders x %d samples x %d)",
                  sizeof(double) * (size_t)s->R * nsamples * (c->d + 1), (long)s->R, nsamples, c->d);
        return CARMA_ENOMEM;
    }
    long off = 0;
    int rc = mpt_iterate(c, (long)nsamples * thin, 1, thin, &off);
    if (rc == CARMA_OK) {
        e = pt_ens_fetch_samples(s, c->d, nsamples, samples, logposts);
        if (e != hipSuccess) rc = hip_fail(e, "carma_mpt_sample: D2H");
    }
    s->cap = capacity;
    return rc;
}

int carma_mpt_stats(carma_mctx* h, double* accept_rate, double* swap_rate, int reset)
{
    MptState* s = mpt_state(h, "carma_mpt_stats", false);
    if (!s) return CARMA_EINVAL;
    Mctx* c = reinterpret_cast<Mctx*>(h);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = pt_ens_stats(s, accept_rate, swap_rate, reset);
    if (e != hipSuccess) return hip_fail(e, "carma_mpt_stats");
    return CARMA_OK;
}

long carma_mpt_iterations_done(const carma_mctx* h)
{
    if (!h || !reinterpret_cast<const Mctx*>(h)->mpt) return CARMA_EINVAL;
    return (long)reinterpret_cast<const Mctx*>(h)->mpt->iter;
}

int carma_mpt_logdensity(carma_mctx* h, const double* theta, double* out)
{
    MptState* s = mpt_state(h, "carma_mpt_logdensity", false);
    if (!s) return CARMA_EINVAL;
    if (!theta || !out) {
        set_error("carma_mpt_logdensity: null theta or out");
        return CARMA_EINVAL;
    }
    Mctx* c = reinterpret_cast<Mctx*>(h);
    const size_t nchain = s->nchain(), GUARD = 64;
    // [nc][d] proposals, [nc] results, then GUARD words nobody may write: a kernel whose idle lanes stored would show here
    std::vector<double> res(nchain + GUARD, 0.0);
    const double mark = -12345.678;
    std::fill(res.begin() + nchain, res.end(), mark);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = c->k_res.need(sizeof(double) * (nchain * c->d + nchain + GUARD));
    double *d_th = c->k_res.as<double>(), *d_ll = d_th + nchain * c->d;
    if (e == hipSuccess) e = hipMemcpyAsync(d_th, theta, sizeof(double) * nchain * c->d, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_ll, res.data(), sizeof(double) * res.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_logdens_chains_ms(c, s, d_th, (long)nchain, d_ll, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(res.data(), d_ll, sizeof(double) * res.size(), hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return hip_fail(e, "carma_mpt_logdensity");
    for (size_t k = nchain; k < res.size(); k++)
        if (res[k] != mark) {
            set_error("carma_mpt_logdensity: the kernel wrote past its %zu results", nchain);
            return CARMA_EHIP;
        }
    std::memcpy(out, res.data(), sizeof(double) * nchain);
    return CARMA_OK;
}

int carma_mpt_kernel_name(const carma_mctx* h, char* buf, int len)
{
    if (!h || !buf || len < 1) return CARMA_EINVAL;
    const Mctx* c = reinterpret_cast<const Mctx*>(h);
    const int r = c->p == 1 ? snprintf(buf, len, "k_logdens_car1_chains_ms") : snprintf(buf, len, "k_logdens_carma_chains_ms<%d>", c->p);
    return r > 0 ? CARMA_OK : CARMA_EINVAL;
}

int carma_mpt_run(carma_mctx* h, const int* series, int M, int ntemps, int nreplicas, int sample_size, int burnin, int thin,
                  const double* init, uint64_t seed, double* samples, double* logposts)
{
    int rc = carma_mpt_create(h, series, M, ntemps, nreplicas, nullptr, burnin, seed);
    if (rc == CARMA_OK) rc = carma_mpt_start(h, init);
    if (rc == CARMA_OK) rc = carma_mpt_iterate(h, burnin, 1);                     // Sampler::Run burn-in (samplers.cpp:97)
    if (rc == CARMA_OK) rc = carma_mpt_sample(h, sample_size, thin, samples, logposts);   // :101-108
    return rc;
}

}  // extern "C"
