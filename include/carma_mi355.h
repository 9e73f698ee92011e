/*
 * carma_mi355.h -- C ABI of libcarma_mi355.so, the MI355X (gfx950) implementation of
 * carma_pack's Kalman-filter log-likelihood path.
 *
 * This is the drop-in boundary: each entry point replaces one binding of the reference's
 * Boost.Python module `carmcmc._carmcmc` (src/boost_python_wrapper.cpp:28-101) or the C++
 * method behind it.  Plain pointers and sizes only; vectors are copied, nothing is retained
 * except what a context owns.  All arithmetic is IEEE FP64.
 *
 * Conventions
 *   - return value 0 = success, negative = error (CARMA_E*); carma_last_error() has the text.
 *   - numerical failure is reported IN BAND, exactly as the reference does: a log-density of
 *     -INFINITY for a prior-bound violation or a repeated AR root (the reference's singular Vandermonde solve)
 *     (src/include/carpack.hpp:134-138,154-164), NaN where the reference's arithmetic gives NaN.
 *   - theta layout (src/carpack.cpp:205-207,432): theta[0]=sigma_y, theta[1]=measurement-error
 *     scale, theta[2]=mu, theta[3..3+p) log quadratic-factor coefficients of the AR polynomial,
 *     theta[3+p..3+p+q) same for the MA polynomial.  CAR(1) (p==1): theta[3]=ln(omega), d=4.
 *   - "_dev" entry points take DEVICE pointers (hipMalloc'ed or a torch tensor's data_ptr) and a
 *     hipStream_t passed as void*; they only enqueue work.  The others take host pointers and
 *     return when the result is in host memory.
 *   - There is no CPU fallback: without a usable gfx950 device every compute call fails with
 *     CARMA_ENODEV.
 *   - ILL-CONDITIONED parameter vectors (deliberate, documented deviation).  The reference forms the constants of the
 *     recursion through an LU solve of the Vandermonde system of the AR roots (KalmanFilterp::Reset, src/kfilter.cpp:157-158)
 *     and p-term sums that cancel when roots cluster -- the prior admits roots 1e-4 apart (src/carpack.cpp:330), where
 *     cond(EigenMat) reaches 1e13 and the reference's own arithmetic is 1e-10 ... 1e-3 away from the exact value of its
 *     formulas.  This library evaluates the same quantities by closed-form products: on such
 *     vectors it returns the closed-form value, NOT the LU's -- within 1e-10 of the reference wherever the reference is
 *     itself within 1e-10 of the exact value, and never further from the exact value than the reference elsewhere
 *     (the tests arbitrate such entries against a quad-precision evaluation and print a census per class of chain:
 *     tests/helpers.py parity_census).
 */
#ifndef CARMA_MI355_H
#define CARMA_MI355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CARMA_OK 0
#define CARMA_EINVAL (-22)
#define CARMA_ENODEV (-19)
#define CARMA_ENOMEM (-12)
#define CARMA_EHIP (-5)

#define CARMA_PMAX 7

typedef struct carma_ctx carma_ctx;
typedef struct carma_comm carma_comm;
typedef struct carma_kf carma_kf;

/* Library / device queries. */
const char* carma_version(void);
const char* carma_last_error(void);
int carma_device_count(void);                      /* 0 when no HIP device is visible */

/*
 * Model context == one CAR1 / CARp / CARMA parameter object of the reference
 * (ctors src/include/carpack.hpp:56-72,254-262,289-298,374-379): copies the series, sorts it by
 * time and drops duplicate times (KalmanFilter::init, src/include/kfilter.hpp:43-76), sets the
 * prior bounds (SetPrior, carpack.hpp:201-207: max_freq = 1/min dt, min_freq = 1/(tmax-tmin))
 * and uploads the series to HBM.  p==1 selects CAR(1) (q must be 0); 2<=p<=7 needs q<p.
 * device = HIP device ordinal.  Returns NULL on error.
 */
carma_ctx* carma_ctx_create(const double* time, const double* y, const double* yerr, int n,
                            int p, int q, double max_stdev, int device);
void carma_ctx_destroy(carma_ctx* h);

int carma_ctx_n(const carma_ctx* h);               /* length after sort/dedup */
int carma_ctx_dim(const carma_ctx* h);             /* d = 3+p+q, or 4 for CAR(1) */
int carma_ctx_get_data(const carma_ctx* h, double* time, double* y, double* yerr);
int carma_ctx_get_prior(const carma_ctx* h, double* out3 /* max_stdev, max_freq, min_freq */);
int carma_ctx_set_prior(carma_ctx* h, double max_stdev);          /* SetPrior, carpack.hpp:201 */

/*
 * Batched CARMA_Base::LogDensity (src/include/carpack.hpp:131-176) == getLogDensity
 * (boost_python_wrapper.cpp:51,59,68) for B parameter vectors, theta = [B][d] row-major.
 * ignore_prior != 0 is SetMLE(true) (carpack.hpp:232; skips the CARp bounds only, the log
 * prior is still added, carpack.hpp:173).  out = [B].
 */
int carma_logdensity_batch(carma_ctx* h, const double* theta, int B, int ignore_prior, double* out);
int carma_logdensity_batch_dev(carma_ctx* h, const double* d_theta, int B, int ignore_prior,
                               double* d_out, void* stream);

/*
 * CarmaModel.get_mle (src/carmcmc/carma_pack.py:195-260: `ntrials` separate scipy L-BFGS-B searches, one FFI crossing
 * per function evaluation) as ONE call: B bounded quasi-Newton searches on f(x) = -LogDensity(x) advanced in lock-step
 * -- per iteration one batched launch evaluates the central-difference stencils of every active start, one more eight
 * backtracking step lengths of every start; projected L-BFGS update (memory `mem`), stopping rules of L-BFGS-B
 * (projected gradient <= gtol; relative decrease <= ftol, three iterations in a row after one restart of the memory).
 * x0 = [B][d] starts; lo / hi = [d] box (NULL or non-finite entries = unbounded); maxiter per start; fd_step = relative
 * finite-difference step; ignore_prior as carma_logdensity_batch (SetMLE(true), carma_pack.py:242).
 * Outputs: x = [B][d], fun = [B] (-LogDensity at x), and optionally nit / nfev / status = [B]
 * (0 converged on the gradient, 1 converged on f, 2 maxiter reached, 3 line search failed, 4 no finite value at the
 * start: the objective is non-finite at the projected x0; such a start ends at once with nit 0, fun 1e300 and x the
 * projected x0).  0 and 1 are successes.
 */
int carma_mle_batched(carma_ctx* h, const double* x0, int B, const double* lo, const double* hi, int maxiter, int mem,
                      double ftol, double gtol, double fd_step, int ignore_prior, double* x, double* fun, int* nit,
                      int* nfev, int* status);

/* Which kernel a launch of B evaluations on this context takes (the launch shape depends on B: DESIGN.md section 3);
 * the name as rocprofv3 lists it, without namespace and argument list.  For measurement scripts. */
int carma_logdensity_kernel_name(const carma_ctx* h, int B, char* buf, int len);

/* Launch-shape switches for measurements and the parity tests (no counterpart in the reference): "WIN_ROWS", "WIN2_EVALS",
 * "PT_ROW_WIN" -- the CARMA_TUNE_* environment variables of the same names give their initial values, read once when the first
 * launch asks; afterwards only this call moves them (process-wide, thread-safe).  CARMA_EINVAL for an unknown name.
 * "CSIM_CHUNK_PATHS": paths per chunk of carma_simulate_cond_* (0: as many as its scratch cap holds; results do not depend on it).
 * "SMOOTH_CHUNK_MODELS": models per chunk of carma_smooth_* (0: as many whole waves as its scratch cap holds; results do not depend on it).
 * "MBAND_SMOOTH_CHUNK_ROWS": parameter vectors per chunk of carma_bands_smooth (0: as many whole waves as its scratch cap holds; results do not depend on it).
 * "MBANDSET_SMOOTH_CHUNK_WAVES": waves per chunk of carma_bandset_smooth (0: as many as its scratch cap holds; results do not depend on it).
 * "PT_RAM_WIDE_MIN": smallest chain dimension whose bookkeeping the lane samplers give to the wide kernels (default 17; 4: every chain). */
int carma_tune_set(const char* name, long value);

/*
 * MANY SERIES per launch (no counterpart in the reference, which fits one light curve per CarmaModel): a survey's light
 * curves, each fitted on its own, in one context and in one launch.
 *
 * carma_mctx_create: series s is time / y / yerr [offsets[s], offsets[s+1]) (offsets[0] = 0, non-decreasing); each series is
 *   prepared exactly as carma_ctx_create prepares one (sort, dedup, prior bounds, regular-cadence test) and the records of
 *   all of them are uploaded into one buffer.  max_stdev = [nseries] or NULL for 10 sqrt(var(y_s, ddof=1)) per series.  All
 *   argument errors (including a series with fewer than 2 distinct times, named by its index) are reported before any
 *   device work.  Returns NULL on error.  carma_mctx_n / _get_data / _get_prior: as the carma_ctx_ calls, for series s.
 * carma_mlogdensity_batch: B evaluations, theta = [B][d], evaluation i on series series[i]; out = [B] in the caller's
 *   order.  One evaluation per lane (k_logdens_carma_lane_ms / k_logdens_car1_ms): series s gets the same bits as the
 *   single-series lane kernel on a context of that series alone, whatever else the batch holds.  A series index out of
 *   range is CARMA_EINVAL before any device work.
 * carma_mle_batched_ms: carma_mle_batched with start i on series series[i] and its own box lo / hi = [B][d] (NULL or
 *   non-finite entries = unbounded); every start's evaluations go through carma_mlogdensity_batch, all starts advance in
 *   lock-step in the same launches.  status as carma_mle_batched (0 ... 4; 4 = no finite value at the start).
 * carma_mkfilter: KalmanFilterp::Filter / KalmanFilter1::Filter of M ITEMS in one launch; item i is the model (sigsqr[i],
 *   omega_re_im[i], ma[i]) on series series[i] of the context, whose order p the models share.  Several items may name one
 *   series, a series may have none.  omega_re_im = [M][p][2], roots in any order but closed under conjugation; ma = [M][nma],
 *   1 <= nma <= p, zero padded to p inside; mu = [M] or NULL (0): subtracted from y and added back to the mean; yerr is used
 *   as given.  p = 1: omega_re_im = [M][2] holds the root (-omega, 0) and ma / nma are ignored.  The output is ragged: item
 *   i has n_i = carma_mctx_n(h, series[i]) means and variances at mean / var [off[i], off[i] + n_i), off[0] = 0, off[i+1] =
 *   off[i] + n_i, items in the caller's order (the caller allocates the sum of the n_i); out_offsets = [M+1] or NULL
 *   receives off.  singular = [M] or NULL: 1 where an item has a repeated AR root (its rows are then not meaningful); the
 *   other items are not affected.  One item per lane (kfilter_lane, car1_filter): an item's rows have the bits
 *   carma_kfilter_batch_carma gives for that model on that series alone, whatever else the call holds.
 * carma_mpredict: Predict of the same kind of items, item i at the times tpred[toff[i] .. toff[i+1]) (toff = [M+1],
 *   non-decreasing; an item without times is legal); pmean / pvar are indexed as tpred.  One lane group per (item, time)
 *   (CAR(1): one lane): the bits of carma_predict_carma / carma_predict_car1 on the series centred by mu, plus mu.
 *   singular as above, set by an item's predictions (an item without times reports 0).
 * carma_msmooth: the interpolated light curve of the same kind of items, arguments and outputs as carma_mpredict, by the
 *   one-pass smoother of carma_smooth_* (below): O((n_i + M_i) p^2) per item instead of O(M_i n_i p^2).  A wave takes items that
 *   share (series, list of times), so that its loop over the merged grid is uniform; other items get waves of their own; idle
 *   groups repeat the wave's first item and write nothing.  An item's outputs have the bits carma_smooth_carma /
 *   carma_smooth_car1 gives for that model on that series alone.  Also CARMA_EINVAL: a time that is not finite (item named).
 *   Both: a series index out of range, roots not closed under conjugation, nma outside 1..p, M < 1 and a decreasing toff are
 *   CARMA_EINVAL before any device work, with the item's index in carma_last_error(); the context stays usable.  The
 *   per-call device buffers belong to the context and grow on demand.
 */
typedef struct carma_mctx carma_mctx;
carma_mctx* carma_mctx_create(const double* time, const double* y, const double* yerr, const long* offsets /* [S+1] */,
                              int nseries, int p, int q, const double* max_stdev /* [S] or NULL */, int device);
void carma_mctx_destroy(carma_mctx* h);
int carma_mctx_nseries(const carma_mctx* h);
int carma_mctx_dim(const carma_mctx* h);
int carma_mctx_n(const carma_mctx* h, int s);           /* length of series s after sort/dedup */
int carma_mctx_get_data(const carma_mctx* h, int s, double* time, double* y, double* yerr);
int carma_mctx_get_prior(const carma_mctx* h, int s, double* out3 /* max_stdev, max_freq, min_freq */);
int carma_mlogdensity_batch(carma_mctx* h, const double* theta /* [B][d] */, const int* series /* [B] */, int B,
                            int ignore_prior, double* out /* [B] */);
int carma_mlogdensity_kernel_name(const carma_mctx* h, char* buf, int len);
int carma_mkfilter(carma_mctx* h, const int* series /* [M] */, int M, const double* sigsqr /* [M] */,
                   const double* omega_re_im /* [M][p][2] */, const double* ma /* [M][nma] */, int nma,
                   const double* mu /* [M] or NULL */, double* mean, double* var, long* out_offsets /* [M+1] or NULL */,
                   int* singular /* [M] or NULL */);
int carma_mpredict(carma_mctx* h, const int* series /* [M] */, int M, const double* sigsqr /* [M] */,
                   const double* omega_re_im /* [M][p][2] */, const double* ma /* [M][nma] */, int nma,
                   const double* mu /* [M] or NULL */, const double* tpred, const long* toff /* [M+1] */, double* pmean,
                   double* pvar, int* singular /* [M] or NULL */);
int carma_msmooth(carma_mctx* h, const int* series /* [M] */, int M, const double* sigsqr /* [M] */,
                  const double* omega_re_im /* [M][p][2] */, const double* ma /* [M][nma] */, int nma,
                  const double* mu /* [M] or NULL */, const double* tout, const long* toff /* [M+1] */, double* mean,
                  double* var, int* singular /* [M] or NULL */);
int carma_mle_batched_ms(carma_mctx* h, const double* x0 /* [B][d] */, const int* series /* [B] */, int B,
                         const double* lo /* [B][d] */, const double* hi /* [B][d] */, int maxiter, int mem, double ftol,
                         double gtol, double fd_step, int ignore_prior, double* x, double* fun, int* nit, int* nfev,
                         int* status);

/*
 * ONE PROCESS IN SEVERAL BANDS, with a lag between them (no counterpart in the reference): K bands observe one latent
 * CARMA(p,q) process x(t); band b sees  y = a_b x(t - lag_b) + mu_b + noise,  noise variance measerr_scale yerr^2.  Band 0 is
 * the reference band (lag 0, a = 1, mu = theta[2]).  The parameter vector is theta of carma_ctx (d = 3 + p + q entries; p = 1:
 * ysigma, measerr_scale, mu, log omega) followed by (lag_b, log a_b, mu_b) for b = 1 ... K - 1: dx = d + 3 (K - 1) entries.
 * The log-density is that of the merged series t - lag_b in time order (equal shifted times are legal), plus the prior of the
 * CARMA part with the bounds of band 0; lag_b is flat inside [lag_lo_b, lag_hi_b] and -inf outside (not tested with
 * ignore_prior), log a_b and mu_b are flat, a non-finite band parameter gives -inf.  p = 1 keeps the CAR(1) bounds with
 * ignore_prior, as carma_logdensity_batch does.
 *
 * carma_bands_create: band b is time / y / yerr [offsets[b], offsets[b+1]) (offsets[0] = 0, every band holds at least one
 *   datum, at least 2 in all), sorted and de-duplicated per band as carma_ctx_create does; 1 <= nbands <= CARMA_KBANDS_MAX;
 *   lag_lo / lag_hi = [nbands - 1], finite (may be NULL for one band); max_stdev bounds ysigma.  Band 0 sets max_freq and
 *   min_freq (SetPrior on its times): with a single datum in band 0 no parameter vector lies inside those bounds and only
 *   ignore_prior evaluations are finite.  All argument errors are reported before any device work.  Returns NULL on error.
 * carma_bands_logdensity_batch: B evaluations, theta = [B][dx], out = [B]; one evaluation per lane (k_logdens_carma_mband), each
 *   lane merging the bands in the order ITS lags give.  _dev: device pointers, enqueued on `stream`, no synchronisation.
 * carma_bands_mle_batched: carma_mle_batched on the extended vector: x0 = [B][dx], lo / hi = [dx] (NULL or non-finite entries =
 *   unbounded; the lag entries are cut to the lag boxes of the handle).  fixed_lag = [B][nbands - 1] or NULL: with it the
 *   optimiser runs on the dx - (nbands - 1) other variables and every evaluation of start i is made at the lags fixed_lag[i]
 *   (the lag entries of x0, lo and hi are not read); x = [B][dx] carries those lags unchanged.  status as carma_mle_batched.
 * carma_bands_smooth: the interpolated light curve of band `band` with its variance under B parameter vectors at once: mean and
 *   variance of a_b x(tout - lag_b) + mu_b (noise-free, in that band's units) given ALL the data of all bands, theta = [B][dx],
 *   tout = [M] observer times of that band in any order, repeats allowed.  One vector per lane: each lane merges the bands and
 *   the requested times in the order ITS lags give and walks the N + M points once forward (k_smooth_mband_fwd) and once backward
 *   (k_smooth_mband_bwd; modified Bryson-Frazier), so vectors with different lags share a call -- the optima of a lag profile,
 *   of many starts.  All data count: equal shifted times are legal and none is dropped; a requested time equal to a datum's
 *   shifted time comes behind it.  The prior is never applied (neither the CARMA bounds nor the lag boxes, also for p = 1).
 *   mean / var = [B][M] in the order of tout, or both NULL; band_mean / band_var = [M], the moment-matched equal-weight mixture
 *   over the rows that are not invalid (as carma_smooth_carma), or both NULL; one pair at least.  invalid = [B] or NULL: 1 where a
 *   row has a repeated AR root or a non-finite lag, scale or offset; its mean / var are NaN and it is left out of the mixture.
 *   The variance is returned as computed, never clipped (see carma_smooth_carma).  Returns CARMA_OK; 1 if a row was invalid and
 *   `invalid` is NULL; CARMA_EINVAL before any device work for a null handle, B < 1, M < 1, band outside [0, nbands), a
 *   mismatched pair or a tout that is not finite.  Scratch: 8 (2 p + p / 2 + 5) (N + M) bytes a row, capped at 256 MiB a chunk of
 *   rows ("MBAND_SMOOTH_CHUNK_ROWS" of carma_tune_set forces a chunk size; a row's result does not depend on it).
 */
#define CARMA_KBANDS_MAX 8
typedef struct carma_bands carma_bands;
carma_bands* carma_bands_create(const double* time, const double* y, const double* yerr, const long* offsets /* [K+1] */,
                                int nbands, int p, int q, const double* lag_lo /* [K-1] */, const double* lag_hi /* [K-1] */,
                                double max_stdev, int device);
void carma_bands_destroy(carma_bands* h);
int carma_bands_dim(const carma_bands* h);              /* dx */
int carma_bands_nbands(const carma_bands* h);
int carma_bands_n(const carma_bands* h, int b);         /* length of band b after sort/dedup */
int carma_bands_get_prior(const carma_bands* h, double* out3 /* max_stdev, max_freq, min_freq */);
int carma_bands_logdensity_batch(carma_bands* h, const double* theta /* [B][dx] */, int B, int ignore_prior, double* out);
int carma_bands_logdensity_batch_dev(carma_bands* h, const double* d_theta, int B, int ignore_prior, double* d_out,
                                     void* stream);
int carma_bands_mle_batched(carma_bands* h, const double* x0 /* [B][dx] */, int B, const double* lo /* [dx] */,
                            const double* hi /* [dx] */, const double* fixed_lag /* [B][K-1] or NULL */, int maxiter, int mem,
                            double ftol, double gtol, double fd_step, int ignore_prior, double* x, double* fun, int* nit,
                            int* nfev, int* status);
int carma_bands_smooth(carma_bands* h, const double* theta /* [B][dx] */, int B, int band,
                       const double* tout /* [M], observer times of that band, any order, repeats allowed */, int M,
                       double* mean /* [B][M] or NULL */, double* var /* [B][M] or NULL */,
                       double* band_mean /* [M] or NULL */, double* band_var /* [M] or NULL */,
                       int* invalid /* [B] or NULL */);

/*
 * MANY MULTI-BAND OBJECTS in one handle (no counterpart in the reference): the S objects of a survey field, each ONE process in
 * the same K bands, fitted each on its own -- with the evaluations of all of them in one launch.  K, p and q are shared by the
 * set, so dx is one number; an object that lacks a band belongs to another set.
 *
 * carma_bandset_create: offsets = [S K + 1]; band b of object s is time / y / yerr [offsets[s K + b], offsets[s K + b + 1]).
 *   Every object is prepared exactly as carma_bands_create prepares its one object (sorted and de-duplicated per band, the time
 *   origin the earliest time of ITS bands, the prior bounds from its band 0 and max_stdev[s]; max_stdev NULL: 10 sqrt(var(y))
 *   of band 0 as given, 0 for a single datum): a set of one object holds the records and the prior of a carma_bands handle of
 *   that object.  lag_lo / lag_hi = [S][K - 1] (may be NULL for one band).  The argument checks are those of carma_bands_create
 *   per object, reported before any device work with the object's index in carma_last_error().  Returns NULL on error.
 * carma_bandset_n: data of band b of object s after sort / dedup.  carma_bandset_get_prior: the bounds of object s.
 * carma_bandset_logdensity_batch: B evaluations, theta = [B][dx], evaluation i on object[i], out = [B] in the caller's order.
 *   One wave per workgroup on ONE object (k_logdens_carma_mband_ms): 64 evaluations of an object a wave, the longest object
 *   first; an object with m evaluations in a call takes ceil(m / 64) waves, the last padded (a single evaluation: 63 pad
 *   lanes).  An evaluation has the bits carma_bands_logdensity_batch gives it on a handle of its object alone, whatever else
 *   the call carries.  An object[i] outside [0, S) is CARMA_EINVAL before any device work and names i; the handle stays
 *   usable.  B = 0 is CARMA_OK.  The per-call device and pinned buffers belong to the handle and grow on demand.
 * carma_bandset_mle_batched: carma_bands_mle_batched with start i on object[i] and its own box lo[i], hi[i] ([B][dx]; NULL or
 *   non-finite entries = unbounded): the lag entries are cut to the lag boxes of object[i], and a start of which that leaves
 *   nothing is CARMA_EINVAL and named (not with fixed_lag, which does not read them).  fixed_lag = [B][K - 1] or NULL, as
 *   carma_bands_mle_batched.  Every optimiser step is ONE carma_bandset_logdensity_batch over the active starts of all objects; a
 *   start's x, fun, nit and status are those of carma_bands_mle_batched on its object alone (nfev may differ: how many stencils
 *   ride along with a line search depends on the number of starts in flight).
 * carma_bandset_smooth: carma_bands_smooth of B ROWS on any objects of the set in one call: row i is the curve of band band[i] of
 *   object[i] under theta[i] ([B][dx]) at the observer times tout[toff[i] ... toff[i + 1]) (toff = [B + 1], at least one time a
 *   row; any order, repeats allowed); its results go to mean / var at toff[i] - toff[0], in the caller's order of that row's
 *   times.  The rows that share (object, band, list of times) are a job and fill waves of 64 in the caller's order, a wave
 *   on ONE job (k_smooth_mband_fwd_ms / k_smooth_mband_bwd_ms), the waves with the most points first; one row alone on its
 *   (object, band, times) takes a wave of which 63 lanes are pads.  A row has the bits carma_bands_smooth gives it on a handle of
 *   its object alone, whatever else the call carries.  The semantics are carma_bands_smooth's: the prior is never applied, the
 *   variance is returned as computed, an invalid row (repeated AR root, non-finite lag, scale or offset) is NaN and sets
 *   invalid[i]; returns CARMA_OK, or 1 if a row was invalid and `invalid` is NULL.  CARMA_EINVAL before any device work for a null
 *   handle, B < 1, a null theta / object / band / tout / toff / mean / var, an object[i] outside [0, S) or band[i] outside [0, K)
 *   (row and value named), a toff that does not grow by at least 1 a row, N_s + M_i beyond an int, or a time that is not finite
 *   (row and position named; the times are read last); the handle stays usable.  Scratch as carma_bands_smooth per wave, capped
 *   at 256 MiB a chunk of waves ("MBANDSET_SMOOTH_CHUNK_WAVES" of carma_tune_set forces the waves of a chunk; a row's result
 *   does not depend on it).
 */
typedef struct carma_bandset carma_bandset;
carma_bandset* carma_bandset_create(const double* time, const double* y, const double* yerr, const long* offsets /* [S*K+1] */,
                                    int nobjects, int nbands, int p, int q, const double* lag_lo /* [S][K-1] */,
                                    const double* lag_hi /* [S][K-1] */, const double* max_stdev /* [S] or NULL */, int device);
void carma_bandset_destroy(carma_bandset* h);
int carma_bandset_nobjects(const carma_bandset* h);
int carma_bandset_nbands(const carma_bandset* h);
int carma_bandset_dim(const carma_bandset* h);          /* dx */
int carma_bandset_n(const carma_bandset* h, int s, int b);
int carma_bandset_get_prior(const carma_bandset* h, int s, double* out3 /* max_stdev, max_freq, min_freq */);
int carma_bandset_logdensity_batch(carma_bandset* h, const double* theta /* [B][dx] */, const int* object /* [B] */, int B,
                                   int ignore_prior, double* out /* [B] */);
int carma_bandset_kernel_name(const carma_bandset* h, char* buf, int len);
int carma_bandset_mle_batched(carma_bandset* h, const double* x0 /* [B][dx] */, const int* object /* [B] */, int B,
                              const double* lo /* [B][dx] */, const double* hi /* [B][dx] */,
                              const double* fixed_lag /* [B][K-1] or NULL */, int maxiter, int mem, double ftol, double gtol,
                              double fd_step, int ignore_prior, double* x, double* fun, int* nit, int* nfev, int* status);
int carma_bandset_smooth(carma_bandset* h, const double* theta /* [B][dx] */, const int* object /* [B] */,
                         const int* band /* [B] */, int B, const double* tout, const long* toff /* [B+1] */, double* mean,
                         double* var, int* invalid /* [B] or NULL */);

/*
 * The parallel-tempering sampler of a MULTI-BAND fit (the carma_mpt_* set on a carma_bands handle, one run): nreplicas independent
 * ladders of ntemps chains on the extended vector [dx], one chain per lane -- the bookkeeping kernels of the large-ensemble
 * sampler (carma_pt_lane.hip; their wide, run-time-dimension form from dx = 17) around a log-density kernel that evaluates every
 * chain with the prior (k_logdens_carma_mband_chains: inside the box the bits of carma_bands_logdensity_batch).  A chain's
 * random streams are keyed by ladder * T + temperature.  dx <= 37, which every legal handle satisfies.
 * THE BAND BOX.  The log-density is flat in log a_b and mu_b, and as log a_b -> -inf the likelihood tends to a positive constant:
 *   the posterior is improper and a hot chain may leave for good.  The sampler confines (log a_b, mu_b) to a box: band_lo /
 *   band_hi = [nbands - 1][2], lo <= hi, outside which a chain's log-density is -inf; both NULL: no box.
 *   carma_bands_pt_default_box writes the box the Python layer uses: log a_b within log 1000 of log(std y_b / std y_0) (0 where that
 *   is undefined), mu_b within [min y_b - span_b, max y_b + span_b], span_b = max y_b - min y_b (max(1, |y_b|) where that is 0).
 * carma_bands_pt_create: temperatures = [ntemps] or NULL (100^(i / (ntemps - 1))).  The initial proposal factor is diagonal: the
 *   CARMA block as carma_pt_create takes it from band 0; per band the lag entry is the median time step of band 0, the log a
 *   entry 0.01, the mu entry sqrt(var y_b / n_b) (0.01 for fewer than 2 data).  CARMA_EINVAL before any device work, with a
 *   message: ntemps outside 1 ... 64, more chains than a launch indexes, dx > 37, a box with lo > hi or one half of it NULL, fewer
 *   than 2 data in band 0.
 * carma_bands_pt_start: init = [dx] or NULL; a finite init row becomes every chain of the run, otherwise every chain draws: the
 *   CARMA part as carma_pt_start draws it on band 0, then every lag uniform in its box, log a_b = log(std y_b / std y_0) (0 where undefined)
 *   and mu_b = mean y_b; candidates that are not finite (or outside the box) are retried in rounds.
 * carma_bands_pt_set_chains / _get_chains: theta = [R][T][dx], logpost = [R][T] (NULL on set: computed, -inf outside the box).
 * carma_bands_pt_get_factor / _set_factor: [R][T][dx*dx].  _iterate / _sample / _stats / _iterations_done: as the carma_mpt_
 *   calls; samples = [R][nsamples][dx].  Every call but _create and _default_box is CARMA_EINVAL before carma_bands_pt_create,
 *   iterate / sample also before the chains have starting values; the handle stays usable.
 * carma_bands_pt_logdensity: the log-densities of chain states theta = [R][T][dx] through the sampler's kernel, out = [R][T].
 * carma_bands_pt_run: create, start, burn-in (adapting), sample.
 */
int carma_bands_pt_default_box(const carma_bands* h, double* band_lo /* [K-1][2] */, double* band_hi /* [K-1][2] */);
int carma_bands_pt_create(carma_bands* h, int ntemps, int nreplicas, const double* temperatures /* [ntemps] or NULL */,
                          int adapt_iters, uint64_t seed, const double* band_lo /* [K-1][2] or NULL */,
                          const double* band_hi /* [K-1][2] or NULL */);
int carma_bands_pt_start(carma_bands* h, const double* init /* [dx] or NULL */);
int carma_bands_pt_set_chains(carma_bands* h, const double* theta /* [R][T][dx] */, const double* logpost /* [R][T] or NULL */);
int carma_bands_pt_get_chains(carma_bands* h, double* theta, double* logpost);
int carma_bands_pt_get_factor(carma_bands* h, double* chol);
int carma_bands_pt_set_factor(carma_bands* h, const double* chol);
int carma_bands_pt_iterate(carma_bands* h, long niter, int do_exchange);
int carma_bands_pt_sample(carma_bands* h, int nsamples, int thin, double* samples /* [R][nsamples][dx] */, double* logposts);
int carma_bands_pt_stats(carma_bands* h, double* accept_rate, double* swap_rate, int reset);
long carma_bands_pt_iterations_done(const carma_bands* h);
int carma_bands_pt_logdensity(carma_bands* h, const double* theta /* [R][T][dx] */, double* out /* [R][T] */);
int carma_bands_pt_kernel_name(const carma_bands* h, char* buf, int len);
int carma_bands_pt_run(carma_bands* h, int ntemps, int nreplicas, int sample_size, int burnin, int thin,
                       const double* init /* [dx] or NULL */, uint64_t seed, const double* band_lo, const double* band_hi,
                       double* samples, double* logposts);

/* ---- the sampler over a SET of multi-band objects (carma_mband_set_pt.hip) ----
 * carma_bands_pt_* for MANY objects of a carma_bandset handle in the same launches.  A RUN is one sampler (nreplicas ladders of
 * ntemps chains on the extended vector) on one object; object[j] is the object of run j (any order, repeats allowed).  The M runs
 * are the ladders j R ... j R + R - 1 of one ensemble of M R ladders, and run j walks, bit for bit, the trajectory those ladders
 * walk under carma_bands_pt_* with M R replicas on a handle of its object alone, whatever its neighbours are.  The log-density
 * kernel gives every run waves of its own (a wave works on one object): ceil(R T / 64) of them.
 *
 * carma_bandset_pt_default_box: carma_bands_pt_default_box of one object.
 * carma_bandset_pt_create: temperatures = [ntemps] or NULL, shared by all runs; band_lo / band_hi = [M][nbands - 1][2], a box per
 *   run, or both NULL: no box.  The initial proposal factor of a run comes from its own object as in carma_bands_pt_create.
 *   CARMA_EINVAL before any device work, with a message that names the run and its object: M < 1, an object index out of range,
 *   more chains (M * nreplicas * ntemps) than a launch indexes, and whatever carma_bands_pt_create refuses for that run.
 * carma_bandset_pt_start: init = [M][dx] or NULL; a run whose row has a finite log-density on its object (inside its box) starts
 *   every chain there, the others draw as carma_bands_pt_start draws, keyed by the chain's slot in the ensemble; the pending
 *   candidates of all runs are evaluated together, one carma_bandset_logdensity_batch a round.
 * carma_bandset_pt_set_chains / _get_chains: theta = [M][R][T][dx], logpost = [M][R][T] (NULL on set: computed, -inf outside the
 *   run's box).  _get_factor / _set_factor: [M][R][T][dx*dx].  _iterate / _sample / _stats / _iterations_done: as the carma_mpt_
 *   calls; samples = [M][R][nsamples][dx], rates = [M][R][T].  Every call but _create and _default_box is CARMA_EINVAL before
 *   carma_bandset_pt_create, iterate / sample also before the chains have starting values; the handle stays usable.
 * carma_bandset_pt_logdensity: the log-densities of chain states theta = [M][R][T][dx], each on its run's object and in its run's
 *   box, through the sampler's kernel; out = [M][R][T].  carma_bandset_pt_kernel_name: that kernel's name.
 * carma_bandset_pt_run: create, start, burn-in (adapting), sample.
 */
int carma_bandset_pt_default_box(const carma_bandset* h, int object, double* band_lo /* [K-1][2] */, double* band_hi /* [K-1][2] */);
int carma_bandset_pt_create(carma_bandset* h, const int* object /* [M] */, int M, int ntemps, int nreplicas,
                            const double* temperatures /* [ntemps] or NULL */, int adapt_iters, uint64_t seed,
                            const double* band_lo /* [M][K-1][2] or NULL */, const double* band_hi /* [M][K-1][2] or NULL */);
int carma_bandset_pt_start(carma_bandset* h, const double* init /* [M][dx] or NULL */);
int carma_bandset_pt_set_chains(carma_bandset* h, const double* theta /* [M][R][T][dx] */,
                                const double* logpost /* [M][R][T] or NULL */);
int carma_bandset_pt_get_chains(carma_bandset* h, double* theta, double* logpost);
int carma_bandset_pt_get_factor(carma_bandset* h, double* chol);
int carma_bandset_pt_set_factor(carma_bandset* h, const double* chol);
int carma_bandset_pt_iterate(carma_bandset* h, long niter, int do_exchange);
int carma_bandset_pt_sample(carma_bandset* h, int nsamples, int thin, double* samples /* [M][R][nsamples][dx] */, double* logposts);
int carma_bandset_pt_stats(carma_bandset* h, double* accept_rate, double* swap_rate, int reset);
long carma_bandset_pt_iterations_done(const carma_bandset* h);
int carma_bandset_pt_logdensity(carma_bandset* h, const double* theta /* [M][R][T][dx] */, double* out /* [M][R][T] */);
int carma_bandset_pt_kernel_name(const carma_bandset* h, char* buf, int len);
int carma_bandset_pt_run(carma_bandset* h, const int* object /* [M] */, int M, int ntemps, int nreplicas, int sample_size,
                         int burnin, int thin, const double* init /* [M][dx] or NULL */, uint64_t seed, const double* band_lo,
                         const double* band_hi, double* samples, double* logposts);

/*
 * The parallel-tempering sampler over MANY SERIES (the carma_pt_* set on a carma_mctx).  A RUN is one sampler -- nreplicas
 * independent ladders of ntemps chains -- on one series of the context; a call takes M runs, series = [M] (an index may repeat,
 * any order).  All runs advance in the same launches: one chain per lane, the bookkeeping kernels of the large-ensemble sampler
 * (carma_pt_lane.hip) and a log-density kernel in which every chain is evaluated on its own series
 * (k_logdens_carma_chains_ms / k_logdens_car1_chains_ms).  Run j owns ladders j R .. j R + R - 1 of ONE ensemble of M R ladders,
 * and a chain's random streams (Philox and starting values) are keyed by its position ladder * T + temperature in that ensemble:
 * run j walks, bit for bit, the trajectory of the block replica0 = j R (carma_pt_shard) of a single-series lane-sampler ensemble
 * on its series, whatever its neighbours are.
 *
 * carma_mpt_create: temperatures = [ntemps] or NULL (100^(i / (ntemps - 1))), shared by all runs; the initial proposal factor of
 *   a run comes from its own series as in carma_pt_create.  CARMA_EINVAL, before any device work and with a message, for M < 1,
 *   ntemps outside 1 ... 64, a series index out of range, or more chains (M * nreplicas * ntemps) than a launch can index.
 * carma_mpt_start: starting values drawn per chain from its series' starting-value distribution, non-finite candidates retried in
 *   rounds (the pending candidates of all runs in one launch); init = [M][d] or NULL: row j is given to every chain of run j when
 *   its log-density on that run's series is finite, else run j draws.
 * carma_mpt_set_chains / _get_chains: theta = [M][R][T][d], logpost = [M][R][T] (NULL on set: computed).
 * carma_mpt_get_factor / _set_factor: [M][R][T][d*d] as carma_pt_get_factor.
 * carma_mpt_iterate / _sample / _stats / _iterations_done: as the carma_pt_ calls; samples = [M][R][nsamples][d], logposts =
 *   [M][R][nsamples], rates = [M][R][T].  The sample buffer is one device allocation; CARMA_ENOMEM names the bytes asked for.
 *   Every call but carma_mpt_create is CARMA_EINVAL before carma_mpt_create, iterate / sample also before the chains have
 *   starting values.
 * carma_mpt_logdensity: the log-densities of chain states theta = [M][R][T][d], each on its run's series, through the sampler's
 *   log-density kernel (the bits of carma_mlogdensity_batch); out = [M][R][T].  carma_mpt_kernel_name: that kernel's name.
 * carma_mpt_run: create, start, burn-in (adapting), sample -- as carma_pt_run.
 */
int carma_mpt_create(carma_mctx* h, const int* series /* [M] */, int M, int ntemps, int nreplicas,
                     const double* temperatures /* [ntemps] or NULL */, int adapt_iters, uint64_t seed);
int carma_mpt_start(carma_mctx* h, const double* init /* [M][d] or NULL */);
int carma_mpt_set_chains(carma_mctx* h, const double* theta /* [M][R][T][d] */, const double* logpost /* [M][R][T] or NULL */);
int carma_mpt_get_chains(carma_mctx* h, double* theta, double* logpost);
int carma_mpt_get_factor(carma_mctx* h, double* chol);
int carma_mpt_set_factor(carma_mctx* h, const double* chol);
int carma_mpt_iterate(carma_mctx* h, long niter, int do_exchange);
int carma_mpt_sample(carma_mctx* h, int nsamples, int thin, double* samples /* [M][R][nsamples][d] */, double* logposts);
int carma_mpt_stats(carma_mctx* h, double* accept_rate, double* swap_rate, int reset);
long carma_mpt_iterations_done(const carma_mctx* h);
int carma_mpt_logdensity(carma_mctx* h, const double* theta /* [M][R][T][d] */, double* out /* [M][R][T] */);
int carma_mpt_kernel_name(const carma_mctx* h, char* buf, int len);
int carma_mpt_run(carma_mctx* h, const int* series /* [M] */, int M, int ntemps, int nreplicas, int sample_size, int burnin,
                  int thin, const double* init /* [M][d] or NULL */, uint64_t seed, double* samples, double* logposts);

/* getLogPrior (carpack.hpp:118-126, wrapper :50,58,67); host arithmetic, one vector. */
double carma_logprior(const carma_ctx* h, const double* theta);

/*
 * KalmanFilterp(time,y,yerr,sigsqr,omega,ma).Filter() + GetMean()/GetVar()
 * (src/include/kfilter.hpp:303-334,126-132; wrapper :91-101).  y is already centred, yerr is
 * used as given; omega_re_im = [p][2]; ma has p entries (zero padded by the caller or here if
 * nma < p, kfilter.hpp:318-320).  The AR roots may come in any order but must be closed under conjugation (real
 * roots, conjugate pairs): anything else is not a real-valued process and is CARMA_EINVAL.  The series is
 * sorted/deduplicated first; *n_out receives the resulting length and mean/var must have room for n values.
 * Returns 1 (and fills nothing useful) for a repeated AR root (singular eigenvector matrix) -- the reference
 * throws std::runtime_error there.
 */
int carma_kfilter_carma(const double* time, const double* y, const double* yerr, int n, int p,
                        double sigsqr, const double* omega_re_im, const double* ma, int nma,
                        double* mean, double* var, int* n_out, int device);
/*
 * Filter() of nmodels CARMA(p, nma-1) models on ONE series in one launch (one model per lane): what
 * a caller looping KalmanFilterp(...).Filter() over posterior samples does (carma_pack.py:374-386 builds
 * one filter per call).  sigsqr [nmodels], omega_re_im [nmodels][p][2], ma [nmodels][nma] (ma[.][0] = 1),
 * mu [nmodels] or NULL (0): subtracted from y and added back to mean, as carma_pack.py:399-400 / :442 do
 * around the filter.  mean, var: [nmodels][n_out] row-major (allocate [nmodels][n]).  singular
 * [nmodels] or NULL: 1 where a model has coincident roots (its rows are then not meaningful: the reference's solve throws).
 */
int carma_kfilter_batch_carma(const double* time, const double* y, const double* yerr, int n, int p,
                              int nmodels, const double* sigsqr, const double* omega_re_im,
                              const double* ma, int nma, const double* mu, double* mean, double* var,
                              int* singular, int* n_out, int device);
/* KalmanFilter1(time,y,yerr,sigsqr,omega).Filter() (kfilter.hpp:222-245; kfilter.cpp:19-48). */
int carma_kfilter_car1(const double* time, const double* y, const double* yerr, int n,
                       double sigsqr, double omega, double* mean, double* var, int* n_out,
                       int device);

/*
 * KalmanFilterp::Predict / KalmanFilter1::Predict (src/kfilter.cpp:218-337, 72-135, 51-69; wrapper
 * :87,98) for M times in ONE launch: conditional mean and variance of the (noise-free) process at
 * tpred[i] given the whole measured series -- interpolation, forecast (tpred > max time) and
 * backcast (tpred < min time).  The reference re-filters the series once per requested time; here
 * every time is one lane group.  Inputs as for carma_kfilter_*; pmean/pvar = [M].  Returns 1 on a
 * singular eigenvector system.
 */
int carma_predict_carma(const double* time, const double* y, const double* yerr, int n, int p,
                        double sigsqr, const double* omega_re_im, const double* ma, int nma,
                        const double* tpred, int M, double* pmean, double* pvar, int device);
int carma_predict_car1(const double* time, const double* y, const double* yerr, int n, double sigsqr,
                       double omega, const double* tpred, int M, double* pmean, double* pvar, int device);

/* The order in which the KalmanFilterp-type entry points want the AR roots -- conjugate pairs adjacent (negative
 * imaginary part first), then the real roots: what CARp::ARRoots emits (src/carpack.cpp:137-172) -- from roots in any
 * order.  They do this themselves; exported for callers that keep per-root quantities aligned.  Host arithmetic.
 * CARMA_EINVAL when the set is not closed under conjugation (to 1e-12).  out = p (re, im) pairs. */
int carma_normalize_roots(int p, const double* omega_re_im, double* out);

/*
 * The same as OBJECTS, as the reference has them (KalmanFilter1 / KalmanFilterp, kfilter.hpp:211-334; wrapper :83-101):
 * carma_kf_create_* copies, sorts and deduplicates the series and uploads it with the model ONCE; Filter and any number
 * of Predict calls then only launch and copy results (the free functions above build such an object per call).
 * carma_kf_n = length after sort/dedup (size of mean/var).  Return codes as above.
 */
carma_kf* carma_kf_create_carma(const double* time, const double* y, const double* yerr, int n, int p, double sigsqr,
                                const double* omega_re_im, const double* ma, int nma, int device);
carma_kf* carma_kf_create_car1(const double* time, const double* y, const double* yerr, int n, double sigsqr,
                               double omega, int device);
void carma_kf_destroy(carma_kf* kf);
int carma_kf_n(const carma_kf* kf);
int carma_kf_filter(carma_kf* kf, double* mean, double* var);
int carma_kf_predict(carma_kf* kf, const double* tpred, int M, double* pmean, double* pvar);

/*
 * carma_process / car1_process (src/carmcmc/carma_pack.py:1148-1259, 1126-1146) for npaths independent paths in ONE
 * launch: exact draws of the process at the n (sorted here) times, value by value from the one-step predictive
 * distribution of the Kalman recursion without measurement error.  Normal variates from the counter-based generator
 * keyed by (seed, path, step): reproducible, and a path does not depend on the batch it is drawn in.
 * out = [npaths][n] (host).  CAR(1): omega = 1 / tau.  Returns 1 on a repeated AR root.
 */
int carma_simulate_carma(const double* time, int n, int p, double sigsqr, const double* omega_re_im,
                         const double* ma, int nma, int npaths, uint64_t seed, double* out, int device);
int carma_simulate_car1(const double* time, int n, double sigsqr, double omega, int npaths, uint64_t seed,
                        double* out, int device);

/*
 * CONDITIONAL simulation of npaths paths on ONE series, path k with a model of its own (sigsqr[k], omega_re_im[k], ma[k],
 * mu[k]): what `for i in range(nsim): ysim[i] = sample.simulate(tsim, bestfit='random')` (src/carmcmc/carma_pack.py:807-837
 * over kfilter.hpp:135-184, one re-filter per time and path) draws, in two launches for all paths.
 * Construction (Matheron's rule):  out_k = f~_k(tsim) + E[f(tsim) | y - mu_k - y~_k] + mu_k,  where
 *   - the series is sorted and deduplicated as carma_kf_create_* does (n_out data remain; fewer than 2: CARMA_EINVAL);
 *   - the merged grid is the stable ascending sort of (the n_out data times, then tsim sorted): n_out + M times, a tsim equal to a
 *     datum behind it; f~_k is carma_simulate_* 's path on that grid (repeated times repeat the value);
 *   - y~_kj = f~_k(t_j) + yerr_j z_kj, and the residual datum is (y_j - mu_k) - y~_kj with yerr_j as given;
 *   - E[.|.] is carma_predict_* of the residual series under model k; the three sums above are rounded one by one, the last
 *     (+ mu_k) is skipped for mu_k = 0.
 * Keys of the counter-based generator: path k uses (seed, path0 + k); its unconditional path takes the normals
 * (step i of the merged grid, idx 0) -- the draws of path path0 + k of carma_simulate_*(merged grid, model k, seed) -- and
 * z_kj is (datum j, idx 1).  A path therefore depends neither on the other paths of the call nor on how the call is cut into
 * chunks (the scratch, 32 n_out + 8 (n_out + M) bytes a path, is capped; "CSIM_CHUNK_PATHS" of carma_tune_set forces a chunk size).
 * omega_re_im = [npaths][p][2], roots in any order but closed under conjugation; ma = [npaths][nma], 1 <= nma <= p, zero padded
 * inside; mu = [npaths] or NULL (0).  out = [npaths][M] in the CALLER's order of tsim.  Optional outputs (NULL to skip), from
 * which every path can be rebuilt with the single-model entry points: uncond = [npaths][n_out + M] (f~ on the merged grid),
 * noise = [npaths][n_out] (z).  singular = [npaths] or NULL: 1 where a path has a repeated AR root (its rows are then not
 * meaningful; other paths are not affected); returns 1 if any path is singular and singular is NULL.  CARMA_EINVAL, before any
 * device work and with the offending path in carma_last_error() where one is at fault: npaths < 1, M < 1, nma outside 1..p,
 * roots not closed under conjugation, sigsqr (omega) not positive, a tsim that is not finite, fewer than 2 distinct data times.
 * CAR(1): omega[k] = 1 / tau_k.
 */
int carma_simulate_cond_carma(const double* time, const double* y, const double* yerr, int n, int p, int npaths,
                              const double* sigsqr, const double* omega_re_im, const double* ma, int nma, const double* mu,
                              const double* tsim, int M, uint64_t seed, unsigned path0, double* out, double* uncond,
                              double* noise, int* singular, int* n_out, int device);
int carma_simulate_cond_car1(const double* time, const double* y, const double* yerr, int n, int npaths,
                             const double* sigsqr, const double* omega, const double* mu, const double* tsim, int M,
                             uint64_t seed, unsigned path0, double* out, double* uncond, double* noise, int* singular,
                             int* n_out, int device);

/*
 * The INTERPOLATED LIGHT CURVE in one pass, for nmodels models on ONE series: mean and variance of the noise-free process at
 * the M times tout given all the data -- what carma_predict_* returns, which filters the whole series again for every time
 * (O(M n p^2)); here a fixed-interval smoother (modified Bryson-Frazier) walks the merged grid of data and requested times once
 * forward and once backward, O((n + M) p^2) per model.  The series is sorted and deduplicated as carma_kf_create_* does (n_out
 * data remain, one is enough); tout in any order, repeats allowed, finite; outputs in the CALLER's order of tout.
 * omega_re_im = [nmodels][p][2], roots in any order but closed under conjugation; ma = [nmodels][nma], 1 <= nma <= p, zero
 * padded inside; mu = [nmodels] or NULL (0): subtracted from y, added back to the mean (skipped for mu = 0).
 * Outputs, each pair optional (NULL, NULL to skip) but one at least:
 *   mean, var = [nmodels][M]   per model.  The variance is a difference (prior variance minus what the data explain) and is
 *                              returned as computed, never clipped: it loses log10(prior / smoothed variance) digits and can come
 *                              out <= 0 by rounding where yerr is tiny against the process.
 *   band_mean, band_var = [M]  the moment-matched Gaussian mixture over the models that are not singular:
 *                              band_mean = (1/K') sum_k mean_k, band_var = (1/K') sum_k (var_k + (mean_k - band_mean)^2), summed
 *                              in ascending k on the device (when only the band is asked for, the [nmodels][M] arrays stay there).
 * singular = [nmodels] or NULL: 1 where a model has a repeated AR root (its rows are not meaningful, it is left out of the band;
 * other models are not affected); returns 1 if any model is singular and singular is NULL.  A model's outputs depend neither on
 * the other models of the call nor on how it is cut into chunks (scratch: 32 G + 32 bytes per grid point and model, G = 2, 4, 8
 * lanes for p <= 2, 4, 7; capped at 256 MiB a chunk; "SMOOTH_CHUNK_MODELS" of carma_tune_set forces a chunk size).
 * CARMA_EINVAL, before any device work and with the offending model in carma_last_error() where one is at fault: nmodels < 1,
 * M < 1, n < 1, nma outside 1..p, roots not closed under conjugation, sigsqr (omega) not positive, a tout that is not finite.
 * CAR(1): omega[k] = 1 / tau_k.
 */
int carma_smooth_carma(const double* time, const double* y, const double* yerr, int n, int p, int nmodels, const double* sigsqr,
                       const double* omega_re_im, const double* ma, int nma, const double* mu, const double* tout, int M,
                       double* mean, double* var, double* band_mean, double* band_var, int* singular, int* n_out, int device);
int carma_smooth_car1(const double* time, const double* y, const double* yerr, int n, int nmodels, const double* sigsqr,
                      const double* omega, const double* mu, const double* tout, int M, double* mean, double* var,
                      double* band_mean, double* band_var, int* singular, int* n_out, int device);

/*
 * CarmaSample post-processing (src/carmcmc/carma_pack.py), one launch per quantity instead of a
 * Python loop over the MCMC samples.
 *
 * carma_sigma_noise_batch == CarmaSample._sigma_noise (carma_pack.py:513-546; the Python twin of CARp::Variance,
 *   src/carpack.cpp:377-409, with sigma = 1): sigma[s] = sqrt(var[s] / Variance(roots_s, ma_s, 1)) for ns samples.
 *   ar_roots_re_im = [ns][p][2], ma_coefs = [ns][nma] (lowest order first, nma <= p), var = [ns]; all host pointers.
 *   A sample whose variance sum is not positive gives NaN, as numpy's sqrt does.
 *
 * carma_psd_band == the numbers behind CarmaSample.plot_power_spectrum (carma_pack.py:548-648) and
 *   Car1Sample.plot_power_spectrum (:950-1035): psd[f][s] = sigma_s^2 |delta_s(2 pi i f)|^2 / |alpha_s(2 pi i f)|^2 on the
 *   nf x ns grid, then np.percentile(psd, percentiles, axis=samples) -- the exact order statistics, numpy's default linear
 *   interpolation.  ar_coefs = [ns][nar] highest order first (np.poly order, nar = p + 1), ma_coefs = [ns][nma] lowest
 *   order first, sigma = [ns], freq = [nf]; band = [nf][nperc] (nperc <= 4; 0: grid only); psd_samples = NULL or
 *   [nf][ns] for the grid itself.  A NaN in a row makes that row's percentiles NaN (np.percentile).
 */
int carma_sigma_noise_batch(int p, int nma, const double* ar_roots_re_im, const double* ma_coefs, const double* var, int ns,
                            double* sigma, int device);
int carma_psd_band(int nar, int nma, const double* ar_coefs, const double* ma_coefs, const double* sigma, int ns,
                   const double* freq, int nf, const double* percentiles, int nperc, double* band, double* psd_samples,
                   int device);

/*
 * carma_mpsd_band == carma_psd_band's percentiles for EVERY series of a sampled set in one call (CarmaModelSet.power_spectrum_band):
 *   nseries series, series s holding the samples sample_start[s] ... sample_start[s + 1] - 1 of the N = sample_start[nseries]
 *   rows of ar_coefs [N][nar] (highest order first), ma_coefs [N][nma] (lowest first) and sigma [N]; sample_start[0] = 0,
 *   strictly increasing.  freq = [nseries][nf], every series its own grid; percentiles [nperc], 1 <= nperc <= 4, in [0, 100];
 *   band = [nseries][nf][nperc].  All host pointers.  One device block and one copy each way per call.  A series of at most
 *   carma_mpsd_fused_max() samples is served by a kernel that forms the spectrum values of a row in LDS, sorts them there and
 *   writes only the percentiles (one launch for all such series, a workgroup per series and carma_mpsd_freq_tile() frequencies);
 *   a longer one goes through carma_psd_band's grid and row-selection kernels inside the same call.  Either way band[s] is what
 *   carma_psd_band gives for series s alone: the same spectrum values to the bit, the exact order statistics, numpy's linear
 *   interpolation, and NaN for every percentile of a row that holds a NaN (that row only).
 *   Bad arguments -- a null pointer, nar / nma outside carma_psd_band's ranges, nseries < 1, nf < 1, a sample_start that does
 *   not start at 0 or does not increase, nperc outside 1 ... 4, a percentile outside [0, 100] -- return CARMA_EINVAL before any
 *   device work.
 */
int carma_mpsd_band(int nar, int nma, const double* ar_coefs, const double* ma_coefs, const double* sigma, const long* sample_start,
                    int nseries, const double* freq, int nf, const double* percentiles, int nperc, double* band, int device);
int carma_mpsd_fused_max(void);
int carma_mpsd_freq_tile(void);

/*
 * carma_chain_diag == the chain diagnostics of a sampled set in one call (MCMCSample.autocorr_timescale / effective_samples,
 * CarmaSample.diagnostics, CarmaModelSet.diagnostics): x = [ngroups][nreplicas][nsamples][d], row-major -- what carma_pt_run and
 * carma_mpt_run return -- every (group, replica) one chain of nsamples rows of d columns.  Per chain and column:
 *   tau     Goodman's `acor` autocorrelation time (MAXLAG 10, WINMULT 5, MINFAC 5: the series is centred, its autocovariances at
 *           lags 0 ... 10 give D = C[0] + 2 sum C[s] and tau = D / C[0]; while tau >= 2 neighbouring values are summed in pairs
 *           and the estimate is repeated on the halved series, and the result is unwound as D = sigma^2 L / 4 level by level)
 *   mean    the plain mean,  sigma: the standard error of the mean that comes with tau
 *   status  0 OK; 1 SHORT: a level had fewer than 50 rows before tau < 2 was reached (the C original silently reports a quarter
 *           of the enclosing level's value there); 2 CONSTANT: C[0] == 0 at level 0; 3 NONFINITE: the column holds a NaN or Inf.
 *           tau = sigma = NaN unless the status is 0.  A negative tau (a short anti-correlated chain) is a legitimate result.
 * rhat = [ngroups][d], or NULL when it is not wanted: split R-hat (BDA3, no rank normalisation) over the 2 nreplicas halves
 * (first and last nsamples / 2 rows) of a group's chains; NaN when nsamples / 2 < 2, when the mean variance W is 0, or when a
 * chain of the group holds a non-finite value in that column.  tau, mean, sigma, status = [ngroups][nreplicas][d].
 * All host pointers.  One device block (the input, the workspace of the halved levels, the results) and one copy each way.  The
 * results are deterministic: the same bits on every call, and a chain's do not depend on the other chains of the call.
 * Bad arguments -- a null x, tau, mean, sigma or status; ngroups, nreplicas or nsamples < 1; d < 1 or d > carma_chain_diag_dmax()
 * (16: the widest parameter vector, 3 + p + q at p = 7) -- return CARMA_EINVAL before any device work.  Short chains are not an
 * argument error.
 */
int carma_chain_diag(const double* x, long ngroups, int nreplicas, long nsamples, int d, double* tau, double* mean, double* sigma,
                     int* status, double* rhat, int device);
int carma_chain_diag_dmax(void);
double carma_chain_diag_kernel_ms(void);    /* device time of the kernels of this process's last successful call; -1 before one */

/*
 * Parallel-tempered Robust-Adaptive-Metropolis sampler == RunCarmaSampler / RunCar1Sampler
 * (src/carmcmc.cpp:30-177; bindings run_mcmc_car1 / run_mcmc_carma, boost_python_wrapper.cpp:76-77)
 * with every chain advanced on the GPU by one persistent kernel (carma_pt.hip).
 *
 *   ntemps     number of tempered chains per ladder = the reference's `nwalkers`; default ladder
 *              T_i = 100^(i/(ntemps-1)) (carmcmc.cpp:92-95), or `temperatures[ntemps]` ascending.
 *   nreplicas  number of INDEPENDENT ladders run side by side (the reference runs exactly one);
 *              each yields its own stream of coldest-chain samples.
 *   adapt_iters  the RAM proposal adapts while iteration < adapt_iters (= burn-in, carmcmc.cpp:149).
 *   seed       counter-based RNG key; runs are reproducible (the reference seeds with time(NULL)).
 *
 * carma_pt_run does the whole Sampler::Run (src/samplers.cpp:57-115): starting values (user
 * `init` honoured only when ninit == d and its posterior is finite, else drawn from the
 * reference's starting-value distribution until finite), `burnin` iterations, then sample_size
 * saves of the coldest chain every `thin` iterations.  samples = [nreplicas][sample_size][d],
 * logposts = [nreplicas][sample_size] (host pointers).
 * The finer-grained calls expose the same machinery for chunked runs, benchmarks and for a
 * temperature ladder sharded across GPUs (carma_pt_shard gives the local block its global
 * temperature / replica indices so RNG streams and swap decisions line up across ranks;
 * carma_pt_bind_state lets the caller own the theta/logpost device buffers so that boundary
 * chains can be exchanged with RCCL send/recv between iterations).
 */
int carma_pt_run(carma_ctx* h, int ntemps, int nreplicas, int sample_size, int burnin, int thin,
                 const double* init, int ninit, uint64_t seed, double* samples, double* logposts);

/* ntemps: the ladder must fit ONE workgroup of the fall-back kernel (k_pt: 8 chains per wave at p >= 5, at most 1024
 * threads and 160 KiB of LDS) -- up to 88 temperatures at CARMA(5,3), 52 at CARMA(7,6); longer ladders are CARMA_EINVAL
 * with the sizes in carma_last_error() (the reference's own runs use about ten), or are split into blocks over
 * ranks (carma_pt_shard). */
int carma_pt_create(carma_ctx* h, int ntemps, int nreplicas, const double* temperatures,
                    int adapt_iters, uint64_t seed);
int carma_pt_shard(carma_ctx* h, int ntemps_global, int slot0, int replica0);
int carma_pt_bind_state(carma_ctx* h, double* d_theta /* [R][T][d] */, double* d_logpost /* [R][T] */);
int carma_pt_start(carma_ctx* h, const double* init, int ninit);
int carma_pt_set_chains(carma_ctx* h, const double* theta /* [R][T][d] */, const double* logpost /* [R][T] or NULL */);
int carma_pt_get_chains(carma_ctx* h, double* theta, double* logpost);
int carma_pt_iterate(carma_ctx* h, long niter, int do_exchange);
int carma_pt_sample(carma_ctx* h, int nsamples, int thin, double* samples, double* logposts);
/* acceptance rate per chain [R][T]; swap_rate[r][i] = accepted swaps between temperatures i and i-1 */
int carma_pt_stats(carma_ctx* h, double* accept_rate, double* swap_rate, int reset);
long carma_pt_iterations_done(const carma_ctx* h);
/* which sampler kernel the context is on: 1 = k_pt_row (one chain per DPP row, ladders spread over workgroups), 0 = k_pt
 * (one workgroup per ladder), 2 = one chain per lane with an iteration as propose kernel + batched log-density launch +
 * finish kernel (carma_pt_lane.hip: ensembles of tens of thousands of chains, ladders of at most 64 temperatures).  A context created on k_pt_row drops to
 * k_pt -- silently -- when a cooperative launch is refused or a cross-workgroup exchange times out; tests assert that it
 * did not.  The kernels draw from the same Philox keys and take the same accept / swap decisions, but round the RAM
 * update and the log-density differently (launch shapes of the same evaluation, 1e-8 apart at most on well-conditioned
 * states): after a fall-back the chains are STATISTICALLY equivalent to, not bit-identical with, an uninterrupted run. */
int carma_pt_kernel_in_use(const carma_ctx* h);
/* which recursion the LAST k_pt_row launch of this process ran on: 0 = one-datum wave pipeline, 1 = windowed pipeline (one-sided),
 * 2 = two-sided windowed pipeline; -1 before the first such launch.  For tests and measurements: the choice (pt_row_plan in
 * carma_shape_plan.h) depends on the whole ladder set's grid, the series (SERIES_WINDOW2_OK) and its length. */
int carma_pt_row_pipeline(void);

/*
 * ONE temperature ladder sharded across the GPUs of a node (one process per GPU): the reference has no counterpart --
 * its ExchangeStep (src/include/steps.hpp:318-362, wired hot -> cold in src/carmcmc.cpp:147-157) swaps two chains of
 * the same process; here the two chains of a pair may live on different GPUs and travel over RCCL / xGMI.
 *
 * carma_comm_*: an RCCL communicator owned by this library (bound at run time to librccl.so.1; no link-time
 * dependency).  Rank 0 calls carma_comm_unique_id and hands the 128 bytes to the other ranks by whatever bootstrap the
 * host program has (torch.distributed broadcast, MPI, a file); every rank then calls carma_comm_create (collective).
 *
 * carma_pt_iterate_sharded: `shards` = the nlocal (normally 1) contexts of this process, each created with
 * carma_pt_create + carma_pt_shard for a contiguous block of temperature slots, consecutive blocks in ascending order;
 * the blocks of all ranks tile the ladder in rank order with the same nlocal everywhere.  Per iteration: the sampler
 * kernel advances every block (RAM steps only), then the ladder's sweep runs hot -> cold over ALL adjacent pairs --
 * inside a block by a sweep kernel, across a block boundary by pack kernel -> ncclSend/ncclRecv of R (d+1) + 1 doubles ->
 * swap kernel -- all on the sampler's stream with no host synchronisation; both sides of a boundary draw the same Philox
 * uniform (seed, hotter chain's global slot, iteration) and take the same decision.  Same pairs, same order, same
 * uniforms as the one-GPU sampler: the chain states equal those of the unsharded run bit for bit.
 * Returns after the last iteration has completed, and after the two sides of every boundary have compared a checksum of
 * their decisions (a mismatch fails the call).  After a failed call the blocks refuse to continue (carma_pt_start /
 * carma_pt_set_chains re-arm them).  comm may be NULL when the process owns the whole ladder as one block.
 */
int carma_comm_unique_id(void* out128);
carma_comm* carma_comm_create(const void* id128, int nranks, int rank, int device);
void carma_comm_destroy(carma_comm* comm);
int carma_comm_rank(const carma_comm* comm);
int carma_comm_size(const carma_comm* comm);
int carma_pt_iterate_sharded(carma_ctx* const* shards, int nlocal, long niter, carma_comm* comm);
/* nsamples x thin more iterations; after every thin-th (and its boundary swaps) the coldest chain of every replica is
 * saved (Sampler::SaveValues, src/samplers.cpp:118-124).  Collective like carma_pt_iterate_sharded; the process that
 * owns temperature 0 receives samples = [R][nsamples][d], logposts = [R][nsamples] (host), the others pass NULL. */
int carma_pt_sample_sharded(carma_ctx* const* shards, int nlocal, int nsamples, int thin, carma_comm* comm,
                            double* samples, double* logposts);
/* boundary swaps this block took part in: proposed = R per boundary and iteration; accepted */
int carma_pt_boundary_stats(carma_ctx* h, unsigned long long* proposed, unsigned long long* accepted);
/* result of the last call's boundary self-check for this block: 1 = both sides of its boundaries folded the same
 * decisions, -1 = they differed (the call failed), 0 = no sharded call yet */
int carma_pt_boundary_check(carma_ctx* h);
/* The sweep over the adjacent pairs INSIDE this block for the iteration just run with do_exchange = 0 (hot -> cold,
 * ExchangeStep, src/include/steps.hpp:318-362): the building block of a sharded iteration for host programs that move
 * the boundary chains themselves (carma_pack_amd/parallel.py over torch.distributed). */
int carma_pt_sweep(carma_ctx* h);

/* ---- debug pair: ties the device sampler step to the reference's arithmetic (tests only; no reference counterpart,
 * the reference's generator is a time-seeded global, src/random.cpp:20) --------------------------------------------
 * carma_pt_debug_draws: the variates chain (replica, temperature) of this block uses at iteration `iter` (counted as
 * AdaptiveMetro::niter_, src/steps.cpp:101), computed on the device by the sampler kernels' own functions: z[d] = the
 * unit proposal (proposal_.Draw, src/steps.cpp:65-69), *u_accept = the Metropolis uniform (src/steps.cpp:48),
 * *u_swap = the uniform of the exchange between this chain and the next colder one (src/include/steps.hpp:333; keyed
 * by the warmer chain's global slot).
 * carma_pt_get_factor / carma_pt_set_factor: chol_factor_ of every chain (src/steps.cpp:32), [R][T][d*d] row-major
 * upper triangular. */
int carma_pt_debug_draws(carma_ctx* h, int replica, int temperature, unsigned long long iter, double* z, double* u_accept,
                         double* u_swap);
int carma_pt_get_factor(carma_ctx* h, double* chol);
int carma_pt_set_factor(carma_ctx* h, const double* chol);

#ifdef __cplusplus
}
#endif
#endif /* CARMA_MI355_H */
