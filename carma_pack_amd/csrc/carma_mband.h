// carma_mband.h -- ONE CARMA(p,q) process seen in K BANDS with a lag, a scale and an offset per band; one evaluation per lane.
//
// Band b observes  y = a_b x(t - lag_b) + mu_b + noise  (noise variance = measerr_scale yerr^2; band 0 is the reference band:
// lag_0 = 0, a_0 = 1, mu_0 = theta[2]).  The parameter vector is the theta of carma_lane.h (d = 3 + p + q entries) followed by
// (lag_b, log a_b, mu_b) for b = 1 ... K - 1: dx = d + 3 (K - 1).  The log-likelihood is that of the merged series
// tau_i = t_i - lag_b(i) in time order -- an order that differs from one parameter vector to the next, so nothing about the series
// is wave-uniform here but its length: every lane walks exactly N = sum_b n_b steps and MERGES the K sorted bands on the fly.
//
//   - the shifted time of every band's head datum lives in a register, heads[KMAX]; the selection is a fully unrolled
//     compare / select over constant indices (the smallest tau wins, on a tie the lower band: results are reproducible);
//   - everything that is read at the index of the SELECTED band -- y and yerr^2 of its head, its position in the record buffer,
//     a_b, mu_b, lag_b -- lives in lane-contiguous work arrays [K][64] (LDS on the device): a runtime-indexed register array would
//     go to scratch;
//   - the selected band's NEXT record is loaded at once and consumed at the end of the step (it is needed at the next selection);
//     every band ends in a sentinel record with t = +inf, which no selection takes and behind which no position moves;
//   - the time step is per lane, so every step computes its own transition factors (lane_factors; no repeated-dt shortcut).
//
// Filter step, in the coordinates of lane_filter (carma_lane.h), for a datum of band b at shifted time tau:
//     z <- Phi z, D <- Phi D Phi^T by dt = tau - tau_previous,  w = D h,  k = w + c
//     var = a^2 (s0 + h.w) + e scale,   innov = (y - mu_b) - a (h.z)
//     z <- z + a k innov / var,         D <- D - a^2 k k^T / var
// Equal shifted times are legal: dt = 0 gives Phi = I exactly (cexp_step_tab / exp_neg_tab at 0).
// Plain C++ over doubles: compiled for the host by the test harness as well (tests/emu/emu_mband.cpp).
#pragma once
#include "carma_lane.h"
#include "carma_prep.h"   // mband_pack, the packer of the records this filter reads (host only)

namespace carma {

constexpr int MBAND_KMAX = 8;        // CARMA_KBANDS_MAX of include/carma_mi355.h
constexpr int MBAND_LANES = 64;      // lanes of a work array row
constexpr double MBAND_LAG_MAX = 1e300;   // a lag beyond it counts as non-finite (t - lag must stay finite)

// The per-lane work arrays of an evaluation, [K][MBAND_LANES] each, already offset by the lane: band b at [b * MBAND_LANES].
struct MbandWork {
    double *y, *e2;                  // head datum of every band
    double *a, *mu, *lag;            // band parameters
    int* pos;                        // position of every band's head in the record buffer
    const int* boff;                 // [K + 1], shared by the lanes: band b is records [boff[b], boff[b + 1]), the last a sentinel
    static constexpr size_t bytes(int K) { return (size_t)K * MBAND_LANES * (5 * sizeof(double) + sizeof(int)); }
};

// Dynamic LDS of a one-wave workgroup whose lanes merge `nstreams` streams (the K bands; the smoother's forward kernel adds the
// requested times as stream K): the math tables, the work arrays [5][nstreams][64] doubles and [nstreams][64] ints, the band
// offsets padded to 16 ints.  Every carve is a multiple of 16 bytes.  mband_lds_carve lays out what this counts.
constexpr size_t mband_lds_bytes(int nstreams) { return sizeof(double) * MATH_TAB_N + MbandWork::bytes(nstreams) + sizeof(int) * 16; }

#if defined(__HIPCC__)
// THE carve of that block, for every kernel of the multi-band path: s_dyn is the base of dynamic LDS; boff = [.][K + 1] are the
// band offsets in global memory, row obj those of the wave's object (0 where a launch has one object).  All lanes of the workgroup
// call it: it fills the tables, copies the object's offsets and runs the barrier.  wk comes back offset by the lane; the return
// value is the tables of the table-based exp / sincos (carma_math.h).
CARMA_DEV const double* mband_lds_carve(double* s_dyn, int nstreams, int K, int lane, const int* boff, long obj, MbandWork& wk)
{
    const size_t KL = (size_t)nstreams * MBAND_LANES;
    double* s_tab = s_dyn;
    double* s_work = s_dyn + MATH_TAB_N;
    int* s_pos = reinterpret_cast<int*>(s_work + 5 * KL);
    int* s_boff = s_pos + KL;
    math_tab_fill(s_tab);
    if (lane <= K) s_boff[lane] = boff[obj * (K + 1) + lane];
    __syncthreads();
    wk.y = s_work + lane;
    wk.e2 = s_work + KL + lane;
    wk.a = s_work + 2 * KL + lane;
    wk.mu = s_work + 3 * KL + lane;
    wk.lag = s_work + 4 * KL + lane;
    wk.pos = s_pos + lane;
    wk.boff = s_boff;
    return s_tab;
}
#endif

// Reset + N merged Updates -> log-likelihood sum (no prior).  rec: {t, y, yerr^2, -} of all bands (MbandWork::boff);
// wk.a / wk.mu / wk.lag are set by the caller, the heads by this function.
template <int P>
CARMA_DEV double lane_filter_mband(const LaneModel<P>& m, bool anyreal, const double* tab, const double4* __restrict__ rec, int K,
                                   int N, const MbandWork& wk)
{
    constexpr int NT = P * (P + 1) / 2;
    constexpr int PE = P & ~1;
    constexpr int L = MBAND_LANES;
    const double inf = 1.0 / 0.0;
    double heads[MBAND_KMAX];
#pragma unroll
    for (int b = 0; b < MBAND_KMAX; b++) {
        heads[b] = inf;
        if (b < K) {                                         // (wave-uniform)
            const int p0 = wk.boff[b];
            const double4 r = rec[p0];
            heads[b] = r.x - wk.lag[b * L];
            wk.y[b * L] = r.y;
            wk.e2[b * L] = r.z;
            wk.pos[b * L] = p0;
        }
    }
    double d[NT];                                            // D after the update of the previous datum
    double zu[P];                                            // z after it
#pragma unroll
    for (int i = 0; i < NT; i++) d[i] = 0.0;
#pragma unroll
    for (int r = 0; r < P; r++) zu[r] = 0.0;
    LogLikAcc acc;
    acc.init();
    double tau_prev = 0.0;
    for (int s = 0; s < N; s++) {
        // --- the band whose head has the smallest shifted time; ties: the lower band
        int b = 0;
        double tau = heads[0];
#pragma unroll
        for (int j = 1; j < MBAND_KMAX; j++) {
            const bool lt = heads[j] < tau;
            tau = lt ? heads[j] : tau;
            b = lt ? j : b;
        }
        const double yb = wk.y[b * L], eb = wk.e2[b * L], ab = wk.a[b * L], mub = wk.mu[b * L], lagb = wk.lag[b * L];
        // --- advance that band: its next record is fetched now and used at the end of the step (never past the sentinel)
        const int last = wk.boff[b + 1] - 1;
        const int pn = wk.pos[b * L] < last ? wk.pos[b * L] + 1 : last;
        const double4 rn = rec[pn];
        // --- z <- Phi z, D <- Phi D Phi^T over dt (the first datum: dt = 0 on z = 0, D = 0)
        const double dt = s == 0 ? 0.0 : tau - tau_prev;
        tau_prev = tau;
        double cr[P], sr[P];
        lane_factors<P>(m.wre, m.wim, m.realpair, anyreal, dt, cr, sr, tab);
        double z[P];
#pragma unroll
        for (int r = 0; r < P; r++) z[r] = (r < PE) ? cr[r] * zu[r] - sr[r] * zu[r ^ 1] : cr[r] * zu[r];
        // mm = d Phi^T for j >= i, and below the diagonal the one entry a pair's even row needs from its partner: (i + 1, i)
        double mm[P][P];
#pragma unroll
        for (int i = 0; i < P; i++) {
#pragma unroll
            for (int j = 0; j < P; j++) {
                const bool need = (j >= i) || (j == i - 1 && (i & 1) && i < PE);
                if (need) {
                    if (j < PE)
                        mm[i][j] = d[tri<P>(i, j)] * cr[j] - d[tri<P>(i, j ^ 1)] * sr[j];
                    else
                        mm[i][j] = d[tri<P>(i, j)] * cr[j];
                } else {
                    mm[i][j] = 0.0;
                }
            }
        }
        double D[NT];
#pragma unroll
        for (int i = 0; i < P; i++) {
#pragma unroll
            for (int j = i; j < P; j++) {
                if (i < PE)
                    D[tri<P>(i, j)] = cr[i] * mm[i][j] - sr[i] * mm[i ^ 1][j];
                else
                    D[tri<P>(i, j)] = cr[i] * mm[i][j];
            }
        }
        // --- w = D h, k = w + c;  var = a^2 (s0 + h.w) + e scale, innov = (y - mu_b) - a h.z
        double k[P];
        double pv = 0.0, pm = 0.0;
#pragma unroll
        for (int i = 0; i < P; i++) {
            double acc_w = 0.0;
#pragma unroll
            for (int j = 0; j < P; j++) acc_w = fma(D[tri<P>(i, j)], m.h[j], acc_w);
            k[i] = acc_w + m.c[i];
            pv = fma(m.h[i], acc_w, pv);
            pm = fma(m.h[i], z[i], pm);
        }
        const double a2 = ab * ab;
        const double var = fma(a2, m.s0 + pv, eb * m.scale);
        const double innov = (yb - mub) - ab * pm;
        acc.add_var(var);
        const double sv = recip(var);
        const double si = sv * innov;
        acc.chi2 += innov * si;
        // --- z <- z + a k innov / var,  D <- D - a^2 k k^T / var
        const double asi = ab * si, a2s = a2 * sv;
#pragma unroll
        for (int r = 0; r < P; r++) zu[r] = fma(k[r], asi, z[r]);
#pragma unroll
        for (int i = 0; i < P; i++) {
            const double t = k[i] * a2s;
#pragma unroll
            for (int j = i; j < P; j++) d[tri<P>(i, j)] = fma(-t, k[j], D[tri<P>(i, j)]);
        }
        // --- the band's new head
        const double tn = rn.x - lagb;
        wk.y[b * L] = rn.y;
        wk.e2[b * L] = rn.z;
        wk.pos[b * L] = pn;
#pragma unroll
        for (int j = 0; j < MBAND_KMAX; j++) heads[j] = (j == b) ? tn : heads[j];
    }
    return acc.total();
}

// Log-density of the extended vector thx = [dx]: the CARMA part as logdensity_lane (lane_model_from_theta, log_prior, -inf outside
// the prior bounds or on a repeated root; p = 1: the bounds of logdensity_car1, which ignore_prior does not lift), lag_b flat inside lagbox = [K - 1][2] (lo, hi;
// not tested with ignore_prior) and -inf outside it, log a_b and mu_b flat; a non-finite band parameter gives -inf.  An
// evaluation that is -inf on its band parameters still walks the N steps, on lag = 0, a = 1, mu = 0.
template <int P>
CARMA_DEV double logdensity_mband_lane(const double* thx, int q, int K, int N, const double4* __restrict__ rec,
                                       const double* lagbox, const Prior& pr, int ignore_prior, const double* tab, const MbandWork& wk)
{
    constexpr int L = MBAND_LANES;
    LaneModel<P> m;
    lane_model_from_theta<P>(thx, q, pr, ignore_prior, m);
    if constexpr (P == 1) {
        const double omega = -m.wre[0], ysigma = thx[0], ms = thx[1];
        m.valid = !((omega > pr.max_freq) || (omega < pr.min_freq) || (ysigma > pr.max_stdev) || (ysigma < 0) || (ms < 0.5) ||
                    (ms > 2.0));
    }
    bool anyreal = false;
#pragma unroll
    for (int i = 0; i < P / 2; i++) anyreal = anyreal || m.realpair[i];
    bool ok = true;
    wk.a[0] = 1.0;
    wk.mu[0] = m.mu;
    wk.lag[0] = 0.0;
    const double* ex = thx + 3 + P + q;
    for (int b = 1; b < K; b++) {                            // (wave-uniform trip count)
        double lag = ex[3 * (b - 1)], a = exp(ex[3 * (b - 1) + 1]), mub = ex[3 * (b - 1) + 2];
        bool good = (fabs(lag) <= MBAND_LAG_MAX) && (a <= 1.7976931348623157e308) && (fabs(mub) <= 1.7976931348623157e308);
        if (!ignore_prior && !(lag >= lagbox[2 * (b - 1)] && lag <= lagbox[2 * (b - 1) + 1])) good = false;
        if (!good) {
            ok = false;
            lag = 0.0;
            a = 1.0;
            mub = 0.0;
        }
        wk.a[b * L] = a;
        wk.mu[b * L] = mub;
        wk.lag[b * L] = lag;
    }
    double ll = lane_filter_mband<P>(m, lane_any(anyreal), tab, rec, K, N, wk);
    ll += log_prior(m.scale, pr.measerr_dof);
    if (m.sing || !m.valid || !ok) ll = -1.0 / 0.0;
    return ll;
}

}  // namespace carma
