// carma_shape_plan.h -- which kernel a call runs: the series flags of a context, the launch plans of the batched log-density
// (CARMA and CAR(1)), the sampler's family, and the plans of the row and the ladder sampler kernels, as pure functions of plain
// values.  The .hip files query the device (DeviceFacts), read the switch table (ShapeSwitches, carma_launch.h), call a planner
// and switch on its plan to name the instantiation.  Nothing here calls HIP, reads the environment or keeps state.
// Standard C++ only: tests/shape/plan_main.cpp exercises it on its own, tests/shape_plan_ref.py restates it.
#pragma once
#include <cstddef>
#include <cstdio>

#include "carma_types.h"

namespace carma {

// a switch nobody set (carma_launch.h: the environment read once, carma_tune_set afterwards)
constexpr long TUNE_UNSET = -0x7fffffffffffffffL - 1;

// What the .hip side found out about the device.
struct DeviceFacts {
    int cus = 256;               // compute units
    int lpc_blocks = 1;          // workgroups of k_logdens_carma_lpc<P,3> a CU holds (registers, LDS), as the runtime counts them
    int row_per_cu = 0;          // workgroups of k_pt_row<P,3> a CU holds; 0: the row sampler does not apply (no cooperative launch, LDS)
};

// The measurement switches, as the table holds them: TUNE_UNSET where nobody set one.  "Unset" below is what each one's
// default reads as: a negative value (a value <= 0 for pt_row_wgs_per_cu), TUNE_UNSET alone for win_rows, win2_evals,
// pt_row_win and lpc_rot.
struct ShapeSwitches {
    long win_rows = TUNE_UNSET, win2_evals = TUNE_UNSET, pt_row_win = TUNE_UNSET;
    long p3l_rows = TUNE_UNSET, lane_min = TUNE_UNSET, lpc_min = TUNE_UNSET, lpc_max = TUNE_UNSET, lpc_rot = TUNE_UNSET;
    long car1_scan_max = TUNE_UNSET;
    long pt_row_wgs_per_cu = TUNE_UNSET, pt_row_rot = TUNE_UNSET, pt_row_xcd_map = TUNE_UNSET;
    long pt_plain = TUNE_UNSET;  // CARMA_PT_PLAIN: 1 plain, 0 producer/consumer
    long pt_ram_wide_min = TUNE_UNSET;   // PT_RAM_WIDE_MIN: smallest chain dimension the wide RAM bookkeeping serves (unset: 17)
};

// ---- series flags (carma_types.h, SERIES_*) ------------------------------------------------------------------------------------
// SERIES_REPEATED_DT: >= 25 % of the time steps dt(k), k = 2 ... n - 1, equal their predecessor
template <class DtAt>
inline bool repeated_dt_rule(long n, DtAt dt)
{
    long rep = 0;
    for (long k = 2; k < n; k++) rep += (dt(k) == dt(k - 1));
    return n > 8 && 4 * rep >= n;
}
// ... of packed records {dt, y, yerr^2, t} (pack_series)
inline bool series_repeated_dt(const double* packed, long n)
{
    return repeated_dt_rule(n, [&](long k) { return packed[4 * (size_t)k]; });
}
// The flag word of n sorted, distinct times under the prior's max_freq, for order p (the window flags for p >= 2 only).
inline int series_flags(const double* t, int n, int p, double max_freq)
{
    int flags = repeated_dt_rule(n, [&](long k) { return t[k] - t[k - 1]; }) ? SERIES_REPEATED_DT : 0;
    if (p < 2) return flags;
    // SERIES_WINDOW_OK (carma_types.h): spans of 16 - p consecutive data against the shortest window the prior admits
    const int ND = 16 - p;
    const double wmin = 0.5 * 600.0 / (6.283185307179586 * max_freq);       // Pipe3LGeom::LIM_RE; the grid halves it at worst
    long over = 0, tot = 0;
    for (int k = 0; k + ND - 1 < n; k++, tot++) over += (t[k + ND - 1] - t[k]) > wmin;
    if (tot > 0 && 10 * over <= tot) flags |= SERIES_WINDOW_OK;
    // SERIES_WINDOW2_OK / _SMALL: chunks of the row with the shortest window against ceil(n / ND)
    long chunks = 0;
    for (int k = 0; k < n; chunks++) {
        int j = k;
        while (j + 1 < n && j + 1 - k < ND && t[j + 1] - t[k] <= wmin) j++;
        k = j + 1;
    }
    const double r = (double)chunks / (double)((n + ND - 1) / ND);
    if (r <= 2.0) flags |= SERIES_WINDOW2_OK;
    if (r <= 3.5) flags |= SERIES_WINDOW2_SMALL;
    return flags;
}
// The series suits the two-sided window pipeline: _OK, or _SMALL where the launch leaves a CU to every workgroup.
inline bool series_two_sided_ok(int flags, bool one_workgroup_per_cu)
{
    return (flags & SERIES_WINDOW2_OK) || ((flags & SERIES_WINDOW2_SMALL) && one_workgroup_per_cu);
}

// ---- batched log-density, CARMA ------------------------------------------------------------------------------------------------
// lanes of the group that holds one evaluation in the lane-group kernels (a row of the state per lane)
constexpr int group_of(int p) { return p <= 2 ? 2 : (p <= 4 ? 4 : 8); }

// Largest launch (in workgroups of four evaluations) that takes the wave pipeline of carma_pipe3l.h: three workgroups
// per CU (measured, tools/tput_probe.py).  CARMA_TUNE_P3L_ROWS overrides it for such measurements.
inline long p3l_max_rows(int cus, const ShapeSwitches& sw)
{
    return sw.p3l_rows >= 0 ? sw.p3l_rows : 3L * cus;      // three workgroups per CU (registers and LDS allow exactly that)
}
// Largest launch (in workgroups of four evaluations) that takes the windowed wave pipeline (carma_pipew.h): one workgroup per CU
// (measured per order at 1024 evaluations, profiles/r05/window_pipeline_v1.txt: 1-10 % ahead of the one-datum pipeline; with two
// or three workgroups per CU that one is ahead).  CARMA_TUNE_WIN_ROWS overrides (0: never, also for the two-sided kernel), so that
// one test process can run both pipelines (carma_tune_set).
inline long win_max_rows(int cus, const ShapeSwitches& sw) { return sw.win_rows != TUNE_UNSET ? sw.win_rows : (long)cus; }
// Largest launch (in EVALUATIONS) that takes the two-sided window pipeline: three workgroups of two evaluations per CU (measured
// per order, profiles/r06/w2_sizes_v1.txt: p = 5 at 1280 / 1536 evaluations 29.6 us against the one-datum pipeline's 35.3 / 35.4,
// p = 7 34.4 against 37.4, p = 3 23.6 against 26.9; at 2048 -- four per CU -- 38.2 against 35.5, 47.8 against 37.5, 31.3 against 27.0).
// CARMA_TUNE_WIN2_EVALS overrides (0: never).
inline long win2_max_evals(int cus, const ShapeSwitches& sw) { return sw.win2_evals != TUNE_UNSET ? sw.win2_evals : 6L * cus; }
// (an override of CARMA_TUNE_WIN_ROWS also lifts the series criterion: the tests force the window pipelines onto series that fail it)
inline bool win_forced(const ShapeSwitches& sw) { return sw.win_rows != TUNE_UNSET; }
// longest series the two-sided kernel keeps in LDS beside its rings (24 bytes a datum; 5000: 137 KiB, one workgroup per CU)
constexpr int W2_MAX_N = 5000;
// Orders whose two-workgroups-per-CU launches take the folded two-pass form of the two-sided kernel (k_logdens_carma_w2, FOLD).
// p = 3 folds as well (one lane per slot, one pass covers the chunk) and was 0.44 us ahead at 1024 evaluations, 17.09 -> 16.64 us --
// short of five times the runs' own spread of 0.09 us, so it keeps the three-pass form.
constexpr bool w2_fold_order(int p) { return p == 5 || p == 7; }
// smallest launch that takes one evaluation per lane (measured: tools/tput_probe.py; CARMA_TUNE_LANE_MIN overrides)
inline long lane_min_evals(int p, int cus, const ShapeSwitches& sw)
{
    if (sw.lane_min >= 0) return sw.lane_min;
    // (p = 7, one producer-wave workgroup per CU: the lane-group kernel keeps 16 385 ... 28 671 evaluations -- 257 us at 24 576
    // against 309 for the lone wave; 374 against 323 at 32 768: profiles/r04/lpc_orders_v1.txt)
    if (p == 7) return 112L * cus;
    return 64L * 4 * cus * 3 / 8;  // 3/8 of a wave per SIMD (24 576 on 256 CUs): 206 vs 212-236 us there
}
// Launches (lpc_min, lpc_max] take the lane kernel with producer waves, k_logdens_carma_lpc<P,3> (measured per order:
// tools/lpc_probe.sh, profiles/r03/lpc_orders_v1.txt).  Below, the lane-group kernels still have at most one wave per SIMD
// and are faster; above -- more than three workgroups per CU, or more than the registers allow (two at p = 5, 6, one at
// p = 7) -- the SIMDs are full either way and the plain lane kernel does the same work without the LDS traffic.
// CARMA_TUNE_LPC_MIN / _MAX override.
inline long lpc_min_evals(int p, int cus, const ShapeSwitches& sw)
{
    if (sw.lpc_min >= 0) return sw.lpc_min;
    // Measured per order (profiles/r04/lpc_orders_v1.txt, round 4: with the table-based exp / sincos and the one-basic-block step
    // the consumer's stream is short enough that for the low orders this kernel wins right above the wave pipeline's range):
    //   p = 2, 3   from 12 x #CUs evaluations (3073):  50 / 62 us flat up to 16 384 against 62-68 / 67-89 (pair kernel, lane groups)
    //   p = 4      from 32 x #CUs (8193):              88 us against 90-93
    //   p >= 5     from 32 x #CUs (8193), as in round 3: below, the lane-group kernel's 104-112 us are ahead of 107-160
    // Round 5, the consumer takes a ring buffer as one basic block (LaneFactorsRing, UNROLLED: 110 -> 92 us at p = 5):
    //   p = 5      from 16 x #CUs (4097): 89-90 us flat against 99-103 for the lane groups (8192: 8.0 -> 9.1e7 evals/s)
    //   p = 4, 6, 7  as before (72 against 71-73; 118 against 104-106; 142 against 109-113: profiles/r05/lpc_min_probe_v1.txt)
    if (p <= 3) return 12L * cus;
    if (p == 5) return 16L * cus;
    return 32L * cus;
}
inline long lpc_max_evals(const DeviceFacts& f, const ShapeSwitches& sw)
{
    if (sw.lpc_max >= 0) return sw.lpc_max;
    return 64L * (f.lpc_blocks < 3 ? f.lpc_blocks : 3) * f.cus;
}

// Launch shape for B evaluations (one table for the launcher and for carma_logdensity_kernel_name)
enum class LdShape { P3L, PC, PLAIN, LANE, LPC, WIN, WIN2, CAR1_SCAN, CAR1_LANE };
struct LdPlan {
    LdShape shape = LdShape::PLAIN;
    int p = 0, G = 0;            // order; lanes per evaluation of the lane-group kernels
    bool repeated_dt = false;    // PLAIN, LANE, LPC: the DTC instantiation
    bool sl = false, ho = false, fold = false;   // WIN2: series in LDS / schedule hand-over / folded producer passes
    bool unrolled = false;       // LPC: <P,3,false,true>
    int pairs = 0;               // PC: consumer + producer pairs per workgroup, 1 or 2
    int waves = 0;               // PLAIN: waves per workgroup, 1 or 4
    int rot = 0;                 // LPC: the part rotation the kernel takes (CARMA_TUNE_LPC_ROT)
    long grid = 0;               // workgroups
    int block = 0;               // threads of a workgroup
};

inline LdPlan logdens_plan(int p, long B, int n, int series_flags, const DeviceFacts& f, const ShapeSwitches& sw)
{
    LdPlan pl;
    pl.p = p;
    pl.G = group_of(p);
    pl.repeated_dt = (series_flags & SERIES_REPEATED_DT) != 0;
    const long cus = f.cus;
    const int EPW = 64 / pl.G;                        // evaluations per wave of the G-lane kernels
    const long waves = (B + EPW - 1) / EPW;
    const long rows = (B + 3) / 4;                    // workgroups with one evaluation per 16-lane DPP row
    const long wgs2 = (B + 1) / 2;                    // workgroups of the two-sided kernel: two evaluations each
    const long lanes = (B + 63) / 64;
    if (B <= win2_max_evals(f.cus, sw) && win_max_rows(f.cus, sw) > 0 && n >= 16 &&
        (series_two_sided_ok(series_flags, wgs2 <= cus) || win_forced(sw))) {
        pl.shape = LdShape::WIN2;                     // (CARMA_TUNE_WIN_ROWS = 0: no window pipeline of either kind)
        pl.sl = n <= W2_MAX_N;                        // (longer: from global memory, the rings alone in LDS)
        pl.ho = pl.sl && wgs2 > cus;
        // two workgroups per CU, odd orders: two folded producer passes and a light wave beside the neighbour's recursion wave
        pl.fold = pl.ho && w2_fold_order(p) && wgs2 <= 2 * cus;
        pl.grid = wgs2, pl.block = 256;
    } else if (rows <= win_max_rows(f.cus, sw) && n >= 8 && ((series_flags & SERIES_WINDOW_OK) || win_forced(sw))) {
        pl.shape = LdShape::WIN;
        pl.grid = rows, pl.block = 256;
    } else if (rows <= p3l_max_rows(f.cus, sw) && n >= 8) {
        // covariance wave + mean wave + two producer waves per four evaluations, co-rotating frame
        // (carma_pipe3l.h); 42 KiB of LDS: up to three workgroups per CU
        pl.shape = LdShape::P3L;
        pl.grid = rows, pl.block = 256;
    } else if (B > lpc_min_evals(p, f.cus, sw) && B <= lpc_max_evals(f, sw) && n >= 8) {
        pl.shape = LdShape::LPC;
        // (up to one workgroup per CU its UNROLLED instantiation, <P,3,false,true>: the same kernel, the same bits)
        pl.unrolled = !pl.repeated_dt && B <= 64 * cus;
        pl.rot = (int)(sw.lpc_rot != TUNE_UNSET ? sw.lpc_rot : 0x0202);
        pl.grid = lanes, pl.block = 256;
    } else if (B >= lane_min_evals(p, f.cus, sw)) {
        // (half-filled waves -- 32 evaluations per wave, twice the waves -- are no faster per wave: an FP64 instruction
        // takes its four cycles whatever the execution mask; 65 536 evaluations 344 vs 233 us)
        pl.shape = LdShape::LANE;
        pl.grid = lanes, pl.block = 64;
    } else if (waves <= 512 && n >= 8) {
        // few evaluations in flight: one wave's instruction stream is the run time, so split it (consumer + rho producer,
        // carma_ring.h).  Beyond 512 waves (two rounds of workgroups) the plain kernel with pair-shared exp/sincos is
        // ahead: 104 vs 111 us at 6144 evaluations (tools/midrange_probe.py)
        pl.shape = LdShape::PC;
        pl.pairs = waves <= 256 ? 1 : 2;
        pl.grid = (waves + pl.pairs - 1) / pl.pairs, pl.block = 128 * pl.pairs;
    } else {
        // spread the waves over as many CUs as possible (1 wave per workgroup) until the chip is covered
        pl.shape = LdShape::PLAIN;
        pl.waves = waves <= 2048 ? 1 : 4;
        pl.grid = (waves + pl.waves - 1) / pl.waves, pl.block = 64 * pl.waves;
    }
    return pl;
}

// ---- batched log-density, CAR(1) -----------------------------------------------------------------------------------------------
// up to 48 evaluations per CU the series is cut across a wave's lanes (k_logdens_car1_scan); beyond, the lanes are worth more
// as evaluations (CARMA_TUNE_CAR1_SCAN_MAX overrides: measured, tools/car1_probe.py)
inline LdPlan logdens_plan_car1(long B, int n, int cus, const ShapeSwitches& sw)
{
    LdPlan pl;
    pl.p = 1;
    const long smax = sw.car1_scan_max >= 0 ? sw.car1_scan_max : 48L * cus;   // (n = 270: 39 against 45 us at 12 288, 52 against 45 at 16 384)
    // (both forms' times are proportional to the series' length: the break-even does not move with it)
    const bool scan = B <= smax && n >= 64;
    pl.shape = scan ? LdShape::CAR1_SCAN : LdShape::CAR1_LANE;
    pl.grid = scan ? B : (B + 63) / 64, pl.block = 64;
    return pl;
}

// The kernel of a plan as rocprofv3 prints it, up to the namespace and the argument list -- the FAMILY: the instances of
// k_logdens_carma_w2 and the unrolled one of k_logdens_carma_lpc give the same bits and share a name (bench.py matches counter
// files on it), and CAR(1)'s parallel-in-time form goes by k_logdens_car1.
inline int logdens_plan_name(const LdPlan& pl, char* buf, int len)
{
    const char* dtc = pl.repeated_dt ? ",true" : "";
    switch (pl.shape) {
        case LdShape::WIN: return snprintf(buf, len, "k_logdens_carma_w<%d>", pl.p);
        case LdShape::WIN2: return snprintf(buf, len, "k_logdens_carma_w2<%d>", pl.p);
        case LdShape::P3L: return snprintf(buf, len, "k_logdens_carma_p3l<%d>", pl.p);
        case LdShape::PC: return snprintf(buf, len, "k_logdens_carma_pc<%d,%d,%d>", pl.p, pl.G, pl.pairs);
        case LdShape::PLAIN: return snprintf(buf, len, "k_logdens_carma<%d,%d,%d%s>", pl.p, pl.G, pl.waves, dtc);
        case LdShape::LANE: return snprintf(buf, len, "k_logdens_carma_lane<%d%s>", pl.p, dtc);
        case LdShape::LPC: return snprintf(buf, len, "k_logdens_carma_lpc<%d,3%s>", pl.p, dtc);
        case LdShape::CAR1_SCAN:
        case LdShape::CAR1_LANE: return snprintf(buf, len, "k_logdens_car1");
    }
    return -1;
}

// ---- sampler family (carma_pt_create) ------------------------------------------------------------------------------------------
enum class PtFamily { LADDER = 0, ROW = 1, LANE = 2 };        // as carma_pt_kernel_in_use reports them
// CARMA_PT_KERNEL: unset, "ladder", "lane", anything else (the tests say "row")
enum class PtForce { NONE, LADDER, ROW, LANE };

// Workgroups of the row sampler the device holds at once: what registers (168 -> three waves per SIMD) and LDS allow per CU, as the
// runtime counts them (DeviceFacts::row_per_cu) -- the cooperative launch checks the same thing again.  Beyond that the ladder
// kernel (8 chains per wave) takes over.  CARMA_TUNE_PT_ROW_WGS_PER_CU lowers it (measurements only).
inline long pt_row_capacity(int T, int n, const DeviceFacts& f, const ShapeSwitches& sw)
{
    if (n < 32 || T < 1 || f.row_per_cu < 1) return 0;
    long per_cu = f.row_per_cu;
    if (sw.pt_row_wgs_per_cu > 0 && sw.pt_row_wgs_per_cu < per_cu) per_cu = sw.pt_row_wgs_per_cu;
    if (per_cu > 3) per_cu = 3;
    return (long)f.cus * per_cu;
}

// Kernel choice for R ladders of T temperatures.  The row variant needs every workgroup of the grid resident at the same time
// (its swap step is a cross-workgroup rendezvous); otherwise one workgroup per ladder (k_pt).
// CARMA_PT_KERNEL=ladder|row overrides (row only where it is safe).
// Large ensembles: ONE CHAIN PER LANE, an iteration as the batched log-density launch + a bookkeeping kernel
// (carma_pt_lane.hip).  Which path pays is measured, per order (tools/mcmc_lane_probe.py, profiles/r04/
// mcmc_lane_threshold_v*.txt; 16 temperatures, n = 270):
//   * the ladder kernel k_pt gives a ladder ceil(T G / 64) waves (G = 2 / 4 / 8 lanes per chain for p = 2 / 3-4 / 5-7); its
//     iteration takes twice as long once those are more than the chip has SIMDs -- p = 5: 8193 chains 245 us against 127,
//     p = 3: 32 768 chains 207 against 98 -- so from there on: one chain per lane, whatever the order;
//   * p <= 4, whose batched launch is the producer-wave kernel right above the wave pipeline's range (lpc_min_evals): from
//     16 x #CUs chains (p = 3: 78 us flat up to 16 384 chains against 103-105, p = 4: 88-107 against
//     116; at 3200 ... 4096 chains the ladder kernel's 74 / 79 us are still ahead of 78 / 83), p = 2 from 12 x #CUs (64 us
//     flat against 73-96); p = 5 from 16 x #CUs as well since round 5 (below).
// CARMA_PT_KERNEL=lane forces it (T <= 64), CARMA_TUNE_PT_LANE_MIN = N (lane_min, TUNE_UNSET without) replaces the table by
// "from N chains".
inline PtFamily pt_family(int p, int T, long R, int n, const DeviceFacts& f, const ShapeSwitches& sw, PtForce force, long lane_min)
{
    const long nchain = (long)T * R;
    if (T <= 64) {
        const long cus = f.cus;
        const int G = p == 2 ? 2 : (p <= 4 ? 4 : 8);
        const long ladder_waves = R * ((T * G + 63) / 64);
        bool pays = ladder_waves > 4 * cus;
        // CAR(1): k_pt gives a chain ONE lane for the whole series (44 us per iteration at n = 270 whatever the ensemble), the batched
        // launch cuts the series across a wave (k_logdens_car1_scan: 8 us for 1024 chains) -- 18.6 against 43.8 us per iteration
        // at 16 x 64, 24.8 against 44.1 at 16 x 256, 59.7 against 73.9 at 16 x 2048; only where the parallel-in-time launch has
        // just run out of waves (48 ... 64 x #CUs chains) the ladder kernel is ahead, 46.9 against 51.4 (car1_sampler_v1.txt)
        // (evidence: n = 270, ensembles from 16 x 64.  Below 64 data the batched launch has no parallel-in-time scan -- one
        // evaluation per lane, logdens_plan_car1 -- and a small ladder such as run_mcmc_car1's default ~10 chains would pay 2-3
        // launches per iteration with nothing parallel to hide them: those keep the persistent k_pt.)
        if (p == 1) pays = n >= 64 && nchain >= 64 && !(nchain > 48 * cus && nchain <= 64 * cus);
        // (p = 3 from 12 x #CUs as well since round 5: 70 us against the ladder kernel's 72.6 at 3200 / 4096 chains; p = 4: 83 against 75,
        // p = 6, 7 at 4608 ... 8192 chains: 150 / 172 against 130 / 138 -- mcmc_lane_threshold_v3.txt)
        if (p == 2 || p == 3) pays = pays || nchain > 12 * cus;
        if (p == 4) pays = pays || nchain > 16 * cus;
        // p = 5 (round 5): its batched launch is the producer-wave kernel from 4 097 evaluations since the consumer takes a ring buffer
        // at a time (89 us) -- 111-112 us per iteration flat for 4 352 ... 8 192 chains against the ladder kernel's 122-125 (which does
        // 80 us up to 4 096 chains, against 91: profiles/r05/mcmc_lane_threshold_v1.txt, _v2.txt)
        if (p == 5) pays = pays || nchain > 16 * cus;
        if (lane_min != TUNE_UNSET) pays = nchain >= lane_min;
        if (force == PtForce::LANE || (force == PtForce::NONE && pays)) return PtFamily::LANE;
    }
    if (p >= 2 && force != PtForce::LADDER && pt_row_capacity(T, n, f, sw) >= R * ((T + 3) / 4)) return PtFamily::ROW;
    return PtFamily::LADDER;
}

// ---- lane sampler: the RAM bookkeeping kernels (carma_pt_lane.hip) -------------------------------------------------------------
// Which propose / finish kernels an iteration of the lane sampler launches around K1, for chains of dimension d.
//   FUSED  k_ram_finish<D,true>: the proposal of the following iteration rides on the finish kernel, where that kernel holds the
//          factor, v, the value AND the draws in registers: d <= 12.  Beyond, the fused form spills -- 296 bytes per lane at
//          d = 13, 1136 at d = 16, where it takes 88 us for 16 384 chains against 21 + 27 for the two kernels
//          (profiles/r04/lane_sampler_kernels_p7_v1.txt)
//   SPLIT  k_ram_propose<D> + k_ram_finish<D,false>: 13 <= d <= 16 (RAM_DMAX, the widest single-series vector, 3 + 7 + 6)
//   WIDE   k_ram_propose_wide + k_ram_finish_wide, run-time d: the factor streamed from memory a row at a time, the vectors in
//          LDS.  From d = 17 (a multi-band vector, 3 + p + q + 3 (K - 1) <= RAM_DMAX_WIDE), where no templated kernel exists;
//          PT_RAM_WIDE_MIN lowers the threshold (down to 4) so that the tests run the wide kernels against the templated ones.
//   NONE   no kernel serves d
constexpr int RAM_DMIN = 4, RAM_DMAX = 16, RAM_DMAX_WIDE = 37, RAM_DFUSED_MAX = 12;
constexpr int RAM_WIDE_MIN_DEFAULT = RAM_DMAX + 1;
enum class RamKernels { NONE = 0, FUSED = 1, SPLIT = 2, WIDE = 3 };
inline RamKernels ram_kernels_plan(int d, const ShapeSwitches& sw)
{
    if (d < RAM_DMIN || d > RAM_DMAX_WIDE) return RamKernels::NONE;
    long wide_min = sw.pt_ram_wide_min != TUNE_UNSET ? sw.pt_ram_wide_min : RAM_WIDE_MIN_DEFAULT;
    if (wide_min > RAM_WIDE_MIN_DEFAULT) wide_min = RAM_WIDE_MIN_DEFAULT;   // (nothing but the wide form exists beyond RAM_DMAX)
    if (d >= wide_min) return RamKernels::WIDE;
    return d <= RAM_DFUSED_MAX ? RamKernels::FUSED : RamKernels::SPLIT;
}

// ---- row sampler (k_pt_row) ----------------------------------------------------------------------------------------------------
struct PtRowPlan {
    bool two = false;            // the TWO-SIDED window pipeline (a chain = two rows, ceil(T / 2) workgroups a ladder)
    bool win = false;            // the one-sided window pipeline
    int minw = 2;                // 3: the 168-register build, where three workgroups share a CU
    bool ho = false;             // two-sided: the schedule hand-over, where workgroups share a CU (carma_pipew.h SSCHED)
    bool sl = true;              // two-sided: the series in LDS; without, from global memory
    int wpl = 1;                 // workgroups per ladder
    long grid = 0;
    int rot = 0, xcd_map = 1;    // PtRowSync::rot, ::xcd_map
    bool cooperative = false;
    int pipeline = 0;            // what carma_pt_row_pipeline reports: 0 one-datum, 1 one-sided window, 2 two-sided
};

// R ladders of T temperatures on this device, T_global in the whole (sharded) ladder; lds_global_series: the LDS bytes of a workgroup
// that holds T_global temperatures and the series (pt_row_lds, carma_pt.hip).
inline PtRowPlan pt_row_plan(long R, int T, int T_global, int n, int series_flags, int cus, size_t lds_global_series,
                             const ShapeSwitches& sw)
{
    PtRowPlan pl;
    const long ncu = cus;
    // the TWO-SIDED window pipeline where the WHOLE ladder set's grid in that form is at most two workgroups per CU, the series
    // suits the window pipeline and fits the LDS beside the rings; from T_global, so that a sharded ladder's blocks decide as the
    // one-GPU run does.  CARMA_TUNE_PT_ROW_WIN = 0 / 1 (one-datum / one-sided window) or 2 (two-sided) overrides.
    const long grid2_global = R * (((long)T_global + 1) / 2);
    // the series sits in LDS: up to 1024 data (24 KiB) two workgroups still share a CU; longer ones -- as long as the LDS holds them
    // (~4800 data) -- where the ladder set leaves a CU to every workgroup, e.g. the single ladder of a run_mcmc call
    // -- and any longer series from global memory through the rows' register windows (18.5 against 17.7 us per launch of the README
    // series: the slower way to feed the producers, and the only one there)
    // (from T_global, like every other choice here: a block of a sharded ladder holds fewer temperatures and would fit more)
    pl.sl = n <= 1024 || (grid2_global <= ncu && lds_global_series <= 160 * 1024);
    bool two = grid2_global <= 2 * ncu && series_two_sided_ok(series_flags, grid2_global <= ncu) && n >= 32;
    if (sw.pt_row_win != TUNE_UNSET) two = sw.pt_row_win == 2 && grid2_global <= 2 * ncu && n >= 32;
    pl.wpl = two ? (T + 1) / 2 : (T + 3) / 4;
    pl.grid = R * pl.wpl;
    pl.minw = pl.grid > 2 * ncu ? 3 : 2;                  // the 168-register build only where three workgroups share a CU
    // the windowed pipeline where the WHOLE ladder's grid is at most one workgroup per CU (from T_global: a sharded ladder's blocks
    // decide as the one-GPU run does, so both stay on one arithmetic); CARMA_TUNE_PT_ROW_WIN=0 / 1 overrides (carma_tune_set)
    const long grid_global = R * (((long)T_global + 3) / 4);
    bool win = grid_global <= ncu && (series_flags & SERIES_WINDOW_OK);      // (and the series suits it: carma_types.h)
    if (sw.pt_row_win != TUNE_UNSET) win = sw.pt_row_win != 0;
    pl.win = win && pl.minw < 3;
    pl.two = two && pl.minw < 3;
    pl.ho = pl.grid > ncu;
    pl.pipeline = pl.two ? 2 : (pl.win ? 1 : 0);
    // Which wave plays which part in the workgroups that share a CU (i, i + ncu, i + 2 ncu).  An ordinary launch places
    // them as k_logdens_carma_p3l's are placed (same tables); the workgroups of a COOPERATIVE launch all land with the
    // same wave -> SIMD pattern (tools/ubench/wave_placement.hip with a second argument 1,
    // profiles/r03/wave_placement_coop.txt), so the parts simply trade places: (cov, mean, P0, P1), (P0, P1, cov, mean),
    // (mean, cov, P1, P0) -- every SIMD gets one covariance or mean wave of each kind at most.
    pl.rot = pl.wpl == 1 ? 0x36D2 : 0xB14E;
    if (sw.pt_row_rot >= 0) pl.rot = (int)sw.pt_row_rot;            // (CARMA_TUNE_PT_ROW_ROT, _XCD_MAP: measurements only)
    pl.xcd_map = (pl.wpl > 1 && R % 8 == 0) ? 8 : 1;
    if (sw.pt_row_xcd_map >= 0) pl.xcd_map = (sw.pt_row_xcd_map > 1 && R % sw.pt_row_xcd_map == 0) ? (int)sw.pt_row_xcd_map : 1;
    // the whole ladder (block) in one workgroup: the rendezvous has a single participant, no co-residency needed --
    // an ordinary launch (a cooperative one costs ~2 ms on this stack, which matters when the ladder is sharded
    // across GPUs and every iteration is a launch of its own).  Otherwise a COOPERATIVE launch: the swap step is a rendezvous
    // of the ladder's workgroups through global memory, so the whole grid has to be resident at once.
    pl.cooperative = pl.wpl != 1;
    return pl;
}

// ---- ladder sampler (k_pt) -----------------------------------------------------------------------------------------------------
struct PtLadderPlan {
    bool fits_pc = false;        // the producer/consumer variant fits (and pays: it needs p >= 2)
    int nthr_fit = 0;            // threads and LDS bytes of the largest workgroup a launch may ask for: that variant's where it
    size_t lds_fit = 0;          // fits (carma_pt_create checks them against the device's limits)
    bool pc = false;             // this launch takes the producer/consumer variant
    int maxt = 256;              // the kernel's thread bound: 256 or 1024
    int nthr = 0;                // threads of a workgroup
    size_t lds = 0;              // LDS bytes of a workgroup
};

// One workgroup per ladder of T temperatures, R ladders; ring_bytes: RingGeom<2>::BYTES (the same for every order).
inline PtLadderPlan pt_ladder_plan(int p, int d, int T, long R, int n, int cus, size_t ring_bytes, const ShapeSwitches& sw)
{
    PtLadderPlan pl;
    const int G = p <= 1 ? 4 : group_of(p);
    const int nthr_c = ((T * G + 63) / 64) * 64;
    const size_t per = 4 * (size_t)d + (size_t)d * d;
    const size_t state = ((size_t)T * per + 4 * (size_t)T + (size_t)T * d) * 8 + (size_t)T * 8 + 16;
    const size_t plain_lds = (size_t)nthr_c * 48 + state;
    const size_t with_ring = plain_lds + (size_t)(nthr_c / 64) * ring_bytes;
    pl.fits_pc = p >= 2 && 2 * nthr_c <= 1024 && with_ring <= 150 * 1024;
    pl.nthr_fit = pl.fits_pc ? 2 * nthr_c : nthr_c;
    pl.lds_fit = pl.fits_pc ? with_ring : plain_lds;
    // The producer/consumer variant halves the instruction stream of the chain waves but doubles the wave count: it
    // wins while a CU holds at most one ladder (12.3k vs 8.0k it/s at 16 x 256) and loses once the ladders queue up
    // for the SIMDs (3.1k vs 4.0k it/s at 16 x 1024, tools/mcmc_bigR_probe.py; the plain chain waves share the
    // exp/sincos inside root pairs, RhoPair).  CARMA_PT_PLAIN=0/1 overrides.  It needs a series long enough to amortise the
    // chunk barriers.
    bool plain = R > (long)cus;
    if (sw.pt_plain >= 0) plain = sw.pt_plain == 1;
    pl.pc = pl.fits_pc && n >= 32 && !plain;
    // (plain variant: every chain wave computes its own rho)
    pl.nthr = pl.pc ? 2 * nthr_c : nthr_c;
    pl.lds = pl.pc ? with_ring : plain_lds;
    pl.maxt = pl.nthr <= 256 ? 256 : 1024;
    return pl;
}

}  // namespace carma
