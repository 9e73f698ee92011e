// carma_launch.h -- host-callable launchers implemented in carma_kernels.hip / carma_pt.hip
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <type_traits>

#include "carma_shape_plan.h"
#include "carma_types.h"

namespace carma {

template <int P>
struct GroupOf {
    static constexpr int value = group_of(P);        // (carma_shape_plan.h)
};

// run-time order -> template argument: f(std::integral_constant<int, P>{}) for p = P in 2 ... 7 (CARMA_PMAX), `bad` for any other p.
// CAR(1) has kernels and argument lists of its own and stays with the caller.
template <class R, class F>
inline R for_order(int p, R bad, F&& f)
{
    switch (p) {
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        default: return bad;
    }
}

// compute units of the current device (cached per device)
int device_cus();

// Launch-shape switches that measurements and the parity tests move: ONE table, read from the environment ONCE,
// when the first caller asks, held in atomics, and moved afterwards through carma_tune_set only -- no getenv() in the launch path (it
// raced with setenv() in multi-threaded callers).  TUNE_UNSET (carma_shape_plan.h): the default.  Every entry is CARMA_TUNE_<name>
// and parsed by atol, but PT_ROW_ROT (hexadecimal) and PT_PLAIN (CARMA_PT_PLAIN: "first character is 1").
// CARMA_TUNE_CSIM_CHUNK_PATHS: paths per chunk of the conditional simulation (carma_csim.hip; 0 or unset: as many as its scratch cap holds).
// CARMA_TUNE_SMOOTH_CHUNK_MODELS: models per chunk of the one-pass smoother (carma_smooth.hip; 0 or unset: as many whole waves as its scratch cap holds).
// CARMA_TUNE_MBAND_SMOOTH_CHUNK_ROWS: parameter vectors per chunk of carma_bands_smooth (carma_mband_smooth.hip; 0 or unset: as many whole waves as its scratch cap holds).
// CARMA_TUNE_MBANDSET_SMOOTH_CHUNK_WAVES: waves per chunk of carma_bandset_smooth (carma_mband_set_smooth.hip; 0 or unset: as many as its scratch cap holds).
enum {
    TUNE_WIN_ROWS = 0, TUNE_WIN2_EVALS, TUNE_PT_ROW_WIN, TUNE_CSIM_CHUNK_PATHS, TUNE_SMOOTH_CHUNK_MODELS,
    TUNE_P3L_ROWS, TUNE_LANE_MIN, TUNE_LPC_MIN, TUNE_LPC_MAX, TUNE_LPC_ROT, TUNE_CAR1_SCAN_MAX,
    TUNE_PT_ROW_WGS_PER_CU, TUNE_PT_ROW_ROT, TUNE_PT_ROW_XCD_MAP, TUNE_PT_PLAIN, TUNE_MBAND_SMOOTH_CHUNK_ROWS,
    TUNE_PT_RAM_WIDE_MIN, TUNE_MBANDSET_SMOOTH_CHUNK_WAVES, TUNE_COUNT
};
long tune_get(int which);                    // TUNE_UNSET or the override
int tune_set(const char* name, long value);  // "WIN_ROWS" / "WIN2_EVALS" / "PT_ROW_WIN" / "CSIM_CHUNK_PATHS" / "SMOOTH_CHUNK_MODELS" / "MBAND_SMOOTH_CHUNK_ROWS" / "MBANDSET_SMOOTH_CHUNK_WAVES" (or the full CARMA_TUNE_ name); 0 or -1
ShapeSwitches shape_switches();              // the planners' switches (carma_shape_plan.h) as the table holds them now

// k_smooth_band (carma_smooth.hip) on `st`: the moment-matched equal-weight mixture over the rows of mean / var = [K][M] whose flag
// in singular = [K] is 0 -> bmean / bvar = [M]
hipError_t launch_smooth_band(const double* mean, const double* var, const int* singular, int K, int M, double* bmean, double* bvar,
                              hipStream_t st);

// repeated_dt: a good part of the series' time steps equal their predecessor (regular cadence): the throughput kernels
// then run the variant that re-uses the transition factors of such steps (carma_core.h, RhoInline DTC)
hipError_t launch_logdens_carma(int p, const double* theta, int B, int d, int q, const double4* series, int n,
                                const Prior& pr, int ignore_prior, double* out, hipStream_t st, int series_flags = 0);
// name of the kernel launch_logdens_* picks for B evaluations of a series of n points (as rocprofv3 prints it, up to
// the namespace and the argument list)
int logdens_kernel_name(int p, long B, int n, char* buf, int len, int series_flags = 0);
hipError_t launch_logdens_car1(const double* theta, int B, const double4* series, int n, const Prior& pr, double* out,
                               hipStream_t st);
hipError_t launch_kfilter_carma(int p, const double* om_re_im, const double* ma, double sigsqr, const double4* series,
                                int n, double* mean, double* var, int* singular, hipStream_t st);
hipError_t launch_kfilter_car1(double sigsqr, double omega, const double4* series, int n, double* mean, double* var,
                               hipStream_t st);

// Filter() of B models in one launch (one model per lane): par = [B][3 p + 2] (roots re/im in normalised order, p MA
// coefficients, sigsqr, mu), mv = scratch of 2 n (B + 64) doubles; mean / var = [B][n] (device)
hipError_t launch_kfilter_batch(int p, const double* par, int B, const double4* series, int n, double* mv, int* singular,
                                double* mean, double* var, hipStream_t st);
hipError_t launch_predict_carma(int p, const double* om_re_im, const double* ma, double sigsqr, const double4* series,
                                int n, const double* tpred, int M, double* pmean, double* pvar, int* singular,
                                hipStream_t st);
hipError_t launch_predict_car1(double sigsqr, double omega, const double4* series, int n, const double* tpred, int M,
                               double* pmean, double* pvar, hipStream_t st);

// npaths independent paths of the process at n sorted times (carma_simulate.h); out = [npaths][n]
hipError_t launch_simulate_carma(int p, const double* om_re_im, const double* ma, double sigsqr, const double* times, int n,
                                 int npaths, unsigned seed0, unsigned seed1, unsigned path0, double* out, int* singular,
                                 hipStream_t st);
hipError_t launch_simulate_car1(double sigsqr, double omega, const double* times, int n, int npaths, unsigned seed0,
                                unsigned seed1, unsigned path0, double* out, hipStream_t st);

// The buffers of an ensemble every sampler kernel takes, in the order of the kernels' parameter lists (pt_ens_buffers, carma_host.h,
// fills it): temps [T]; theta [R T][d], logpost [R T], chol [R T][d d]; naccept, nswap [R T]; samples [R][cap][d], sample_lp [R][cap]
struct PtBuffers {
    const double* temps;
    double *theta, *logpost, *chol;
    unsigned *naccept, *nswap;
    double *samples, *sample_lp;
};

// one chunk of the persistent PT sampler kernel (carma_pt.hip)
hipError_t launch_pt(int p, const PtLaunch& L, const double4* series, const Prior& pr, const PtBuffers& b, hipStream_t st);
size_t pt_lds_bytes(int P, int d, int T, int* nthreads_out);
// row variant (one chain per 16-lane DPP row, ladders spread over several workgroups): workgroups of it a CU holds for this
// (p, d, T) as the runtime counts them (DeviceFacts::row_per_cu), 0 if the variant does not apply
int pt_row_per_cu(int p, int d, int T);
int pt_row_last_pipeline();     // 0 / 1 / 2 as carma_pt_row_pipeline (include/carma_mi355.h); -1 before the first launch
hipError_t launch_pt_row(int p, const PtLaunch& L, const PtRowSync& S, const double4* series, const Prior& pr, const PtBuffers& b,
                         hipStream_t st);

// sampler for large ensembles (carma_pt_lane.hip): one chain per lane, an iteration = propose kernel + the batched
// log-density launch above + finish kernel; a ladder's T <= 64 chains are T consecutive lanes.  Enqueues L.niter
// iterations on st.  scratch: pt_lane_scratch_doubles(d, T * R) doubles of device memory (chain-minor working state).
size_t pt_lane_scratch_doubles(int d, long nchain);
hipError_t launch_pt_lane(int p, const PtLaunch& L, double* scratch, const double4* series, const Prior& pr, const PtBuffers& b,
                          int series_flags, bool load_factor, hipStream_t st);
// the same loop with the log-density step ("K1") supplied by the caller: k1(thn [nc][d], nc, ll [nc], st) enqueues the
// log-densities of the nc = R * T proposals (chain-major, chain = ladder * T + temperature) on st
using PtLaneK1 = std::function<hipError_t(const double* thn, long nc, double* ll, hipStream_t st)>;
hipError_t launch_pt_lane_k1(int p, const PtLaunch& L, double* scratch, const PtLaneK1& k1, const PtBuffers& b, bool load_factor,
                             hipStream_t st);
// the lane sampler keeps the proposal factors in its chain-minor working state between calls; this writes them to the chain-major
// array the other entry points read (carma_pt_get_factor, the shard packers): enqueued on st
hipError_t pt_lane_store_factor(int d, int T, int R, double* scratch, double* chol, hipStream_t st);

}  // namespace carma
