// carma_mband_smooth.h -- the interpolated light curve of ONE BAND of a multi-band fit (carma_mband.h) with its variance, in one
// forward and one backward pass per parameter vector; one vector per lane.
//
// The requested times of the output band bo are one more stream in the merge of lane_filter_mband: the host sorts them once
// (a requested time tout sits at tout - lag_bo in lane coordinates, the same shift for all of them, so the host's order holds in
// every lane), stores them as records {tout - t0, caller's slot, -, -} with a sentinel at +inf behind them, and the lane gives
// the stream the index K in its compare / select -- behind every band, so a requested time equal to a datum's shifted time
// comes behind the datum (the rule of smooth_merge).  The walk is exactly ng = N + M steps, wave-uniform.
//
// Forward, at point i with the PREDICTED z, D (the notation of carma_mband.h; the step TO the point by cr, sr):
//     k = D h + c (= P h)      f = s0 + h.(D h) (= h P h)      pm = h.z
//   datum of band b:   F = a_b^2 f + e scale,  s = 1 / F,  innov = (y - mu_b) - a_b pm,  z += a_b k innov s,  D -= a_b^2 s k k^T
//   requested time:    s = 0: z and D pass through
//   and the record {k[P], cr[P], sr of every pair's even member [P / 2], pm, f, s, innov (request: the slot), a_b} is stored.
// Backward (modified Bryson-Frazier in the real lane coordinates; with H = a h^T, gain a s k, L = I - a^2 s k h^T this is
// r <- H^T s innov + L^T r, N <- H^T s H + L^T N L; K = 1, a = 1: the formulas of carma_smooth.h), r = 0, N = 0 behind the
// last point, N symmetric and kept as its upper triangle; at point i:
//     av = N k,  qn = k.av,  hh = k.r
//   requested time:    mean = a_bo (pm + hh) + mu_bo,   var = a_bo^2 (f - qn)   -> the caller's slot
//   datum, g = a_b^2 s:  r <- r + h a_b s (innov - a_b hh),   N <- N - g (h av^T + av h^T) + (g + g^2 qn) h h^T
//   then back over the step that led TO the point:  r <- Phi^T r,  N <- Phi^T N Phi,  (Phi^T x)_j = cr_j x_j - sr_{j^1} x_{j^1}
//   (cr_j x_j alone for the unpaired coordinate).
// The variance is a difference and is returned AS COMPUTED, never clipped (see carma_smooth.h).
//
// Scratch: field q of point i of this lane at sc[i * ps + q * fs] -- on the device [wave][point][field][64], so that every store
// and load of a field is one contiguous 512-byte row of the wave (carma_mband_smooth_plan.h).  A lane reads only what it wrote.
// Plain C++ over doubles: compiled for the host by the test harness as well (tests/emu/emu_mband_smooth.cpp).
#pragma once
#include "carma_mband.h"

namespace carma {

// doubles of a point's record
template <int P>
constexpr int mband_smooth_fields()
{
    return 2 * P + P / 2 + 5;
}

// (lag_b, a_b, mu_b) of band b >= 1 as logdensity_mband_lane reads them, the lag boxes not tested; false: a non-finite one (then
// lag 0, a 1, mu 0)
CARMA_DEV bool mband_band_params(const double* ex, int b, double& lag, double& a, double& mub)
{
    lag = ex[3 * (b - 1)];
    a = exp(ex[3 * (b - 1) + 1]);
    mub = ex[3 * (b - 1) + 2];
    const bool good = (fabs(lag) <= MBAND_LAG_MAX) && (a <= 1.7976931348623157e308) && (fabs(mub) <= 1.7976931348623157e308);
    if (!good) {
        lag = 0.0;
        a = 1.0;
        mub = 0.0;
    }
    return good;
}

// What both passes need of a parameter vector: the model (prior ignored) and the output band's (lag, a, mu).  ok: no repeated
// AR root and every band parameter finite; a vector that is not ok is walked on lag 0, a = 1, mu = 0 in its bad bands.
template <int P>
struct MbandSmoothLane {
    LaneModel<P> m;
    double lag_o, a_o, mu_o;
    bool ok;
};

// wk: the work arrays of the forward pass ([K + 1] rows: the bands, then the requested times), or null (backward pass)
template <int P>
CARMA_DEV void mband_smooth_setup(const double* thx, int q, int K, int bo, MbandSmoothLane<P>& s, const MbandWork* wk)
{
    constexpr int L = MBAND_LANES;
    const Prior none{0.0, 0.0, 0.0, 0.0};
    lane_model_from_theta<P>(thx, q, none, 1, s.m);
    s.ok = !s.m.sing;
    s.lag_o = 0.0;
    s.a_o = 1.0;
    s.mu_o = s.m.mu;
    if (wk) {
        wk->a[0] = 1.0;
        wk->mu[0] = s.m.mu;
        wk->lag[0] = 0.0;
    }
    const double* ex = thx + 3 + P + q;
    for (int b = 1; b < K; b++) {                            // (wave-uniform trip count)
        double lag, a, mub;
        if (!mband_band_params(ex, b, lag, a, mub)) s.ok = false;
        if (wk) {
            wk->a[b * L] = a;
            wk->mu[b * L] = mub;
            wk->lag[b * L] = lag;
        }
        if (b == bo) {
            s.lag_o = lag;
            s.a_o = a;
            s.mu_o = mub;
        }
    }
    if (wk) {
        wk->a[K * L] = 1.0;
        wk->mu[K * L] = 0.0;
        wk->lag[K * L] = s.lag_o;
    }
}

// Forward pass.  rec: the bands' records (wk.boff); req: the M requested times {tout - t0, slot, -, -} in ascending order and the
// sentinel; wk.a / mu / lag are set (mband_smooth_setup), the heads by this function.  sc: field 0 of point 0 of this lane.
template <int P>
CARMA_DEV void lane_smooth_forward_mband(const LaneModel<P>& m, bool anyreal, const double* tab, const double4* __restrict__ rec,
                                         const double4* __restrict__ req, int K, int N, int M, const MbandWork& wk,
                                         double* __restrict__ sc, long fs, long ps)
{
    constexpr int NT = P * (P + 1) / 2;
    constexpr int PE = P & ~1;
    constexpr int L = MBAND_LANES;
    const double inf = 1.0 / 0.0;
    double heads[MBAND_KMAX + 1];
#pragma unroll
    for (int b = 0; b <= MBAND_KMAX; b++) {
        heads[b] = inf;
        if (b <= K) {                                        // (wave-uniform)
            const int p0 = b < K ? wk.boff[b] : 0;
            const double4 r = b < K ? rec[p0] : req[0];
            heads[b] = r.x - wk.lag[b * L];
            wk.y[b * L] = r.y;
            wk.e2[b * L] = r.z;
            wk.pos[b * L] = p0;
        }
    }
    double d[NT];                                            // D after the update of the previous point
    double zu[P];                                            // z after it
#pragma unroll
    for (int i = 0; i < NT; i++) d[i] = 0.0;
#pragma unroll
    for (int r = 0; r < P; r++) zu[r] = 0.0;
    double tau_prev = 0.0;
    const int ng = N + M;
    for (int s = 0; s < ng; s++) {
        // --- the stream whose head has the smallest shifted time; ties: the lower stream, the requested times last
        int b = 0;
        double tau = heads[0];
#pragma unroll
        for (int j = 1; j <= MBAND_KMAX; j++) {
            const bool lt = heads[j] < tau;
            tau = lt ? heads[j] : tau;
            b = lt ? j : b;
        }
        const bool isreq = b == K;
        const double yb = wk.y[b * L], eb = wk.e2[b * L], ab = wk.a[b * L], mub = wk.mu[b * L], lagb = wk.lag[b * L];
        // --- advance that stream: its next record is fetched now and used at the end of the step (never past the sentinel)
        const int last = isreq ? M : wk.boff[b + 1] - 1;
        const int pn = wk.pos[b * L] < last ? wk.pos[b * L] + 1 : last;
        const double4 rn = isreq ? req[pn] : rec[pn];
        // --- z <- Phi z, D <- Phi D Phi^T over dt (the first point: dt = 0 on z = 0, D = 0)
        const double dt = s == 0 ? 0.0 : tau - tau_prev;
        tau_prev = tau;
        double cr[P], sr[P];
        lane_factors<P>(m.wre, m.wim, m.realpair, anyreal, dt, cr, sr, tab);
        double z[P];
#pragma unroll
        for (int r = 0; r < P; r++) z[r] = (r < PE) ? cr[r] * zu[r] - sr[r] * zu[r ^ 1] : cr[r] * zu[r];
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
        // --- w = D h, k = w + c;  f = s0 + h.w,  pm = h.z
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
        const double f = m.s0 + pv;
        const double a2 = ab * ab;
        const double var = fma(a2, f, eb * m.scale);
        const double innov = (yb - mub) - ab * pm;
        const double sv = isreq ? 0.0 : recip(var);
        // --- the record of the point
        double* o = sc + (long)s * ps;
#pragma unroll
        for (int r = 0; r < P; r++) o[r * fs] = k[r];
#pragma unroll
        for (int r = 0; r < P; r++) o[(P + r) * fs] = cr[r];
#pragma unroll
        for (int i = 0; i < P / 2; i++) o[(2 * P + i) * fs] = sr[2 * i];
        double* og = o + (2 * P + P / 2) * fs;
        og[0] = pm;
        og[fs] = f;
        og[2 * fs] = sv;
        og[3 * fs] = isreq ? yb : innov;
        og[4 * fs] = ab;
        // --- z <- z + a k innov s,  D <- D - a^2 s k k^T  (a requested time: z and D as they are)
        const double asi = ab * (sv * innov), a2s = a2 * sv;
#pragma unroll
        for (int r = 0; r < P; r++) zu[r] = isreq ? z[r] : fma(k[r], asi, z[r]);
#pragma unroll
        for (int i = 0; i < P; i++) {
            const double t = k[i] * a2s;
#pragma unroll
            for (int j = i; j < P; j++) d[tri<P>(i, j)] = isreq ? D[tri<P>(i, j)] : fma(-t, k[j], D[tri<P>(i, j)]);
        }
        // --- the stream's new head
        const double tn = rn.x - lagb;
        wk.y[b * L] = rn.y;
        wk.e2[b * L] = rn.z;
        wk.pos[b * L] = pn;
#pragma unroll
        for (int j = 0; j <= MBAND_KMAX; j++) heads[j] = (j == b) ? tn : heads[j];
    }
}

// one point's record in registers
template <int P>
struct MbandSmoothRec {
    double k[P], cr[P], sh[P / 2 + 1];                       // sh: sr of the even member of every pair
    double pm, f, s, v, a;                                   // v: innov at a datum (s != 0), the slot at a requested time
    CARMA_DEV void load(const double* __restrict__ o, long fs)
    {
#pragma unroll
        for (int r = 0; r < P; r++) k[r] = o[r * fs];
#pragma unroll
        for (int r = 0; r < P; r++) cr[r] = o[(P + r) * fs];
#pragma unroll
        for (int i = 0; i < P / 2; i++) sh[i] = o[(2 * P + i) * fs];
        const double* og = o + (2 * P + P / 2) * fs;
        pm = og[0];
        f = og[fs];
        s = og[2 * fs];
        v = og[3 * fs];
        a = og[4 * fs];
    }
};

// Backward pass over the ng records of the forward pass.  pmean / pvar: this vector's M outputs in the caller's order, or null
// (a pad lane); bad: the vector is not ok -- the walk is made all the same and NaN is written.
template <int P>
CARMA_DEV void lane_smooth_backward_mband(const LaneModel<P>& m, double a_o, double mu_o, bool bad, int ng,
                                          const double* __restrict__ sc, long fs, long ps, int M, double* __restrict__ pmean,
                                          double* __restrict__ pvar)
{
    constexpr int NT = P * (P + 1) / 2;
    constexpr int PE = P & ~1;
    const double nan = 0.0 / 0.0;
    double Nm[NT], r[P];
#pragma unroll
    for (int i = 0; i < NT; i++) Nm[i] = 0.0;
#pragma unroll
    for (int i = 0; i < P; i++) r[i] = 0.0;
    // the record of point i - 1 is loaded while point i is worked on (its latency would sit on the dependent chain)
    MbandSmoothRec<P> c;
    c.load(sc + (long)(ng - 1) * ps, fs);
    for (int i = ng - 1; i >= 0; i--) {
        MbandSmoothRec<P> cp;
        cp.load(sc + (long)(i > 0 ? i - 1 : 0) * ps, fs);
        double av[P];
        double qn = 0.0, hh = 0.0;
#pragma unroll
        for (int a = 0; a < P; a++) {
            double t = 0.0;
#pragma unroll
            for (int b = 0; b < P; b++) t = fma(Nm[tri<P>(a, b)], c.k[b], t);
            av[a] = t;
        }
#pragma unroll
        for (int a = 0; a < P; a++) {
            qn = fma(c.k[a], av[a], qn);
            hh = fma(c.k[a], r[a], hh);
        }
        if (c.s == 0.0) {                                    // a requested time (a datum's 1 / F is never 0)
            if (pmean) {
                int slot = (int)c.v;
                slot = slot < 0 ? 0 : (slot >= M ? M - 1 : slot);
                pmean[slot] = bad ? nan : fma(a_o, c.pm + hh, mu_o);
                pvar[slot] = bad ? nan : (a_o * a_o) * (c.f - qn);
            }
        } else {
            const double g = (c.a * c.a) * c.s;
            const double gr = (c.a * c.s) * (c.v - c.a * hh);
            const double coef = fma(g * qn, g, g);
#pragma unroll
            for (int a = 0; a < P; a++) r[a] = fma(m.h[a], gr, r[a]);
#pragma unroll
            for (int a = 0; a < P; a++) {
                const double ha = m.h[a] * coef, ga = g * av[a], gh = g * m.h[a];
#pragma unroll
                for (int b = a; b < P; b++) {
                    double t = fma(-gh, av[b], Nm[tri<P>(a, b)]);
                    t = fma(-ga, m.h[b], t);
                    Nm[tri<P>(a, b)] = fma(ha, m.h[b], t);
                }
            }
        }
        // --- back over the step that led to point i: r <- Phi^T r, N <- Phi^T N Phi;  sr_j = -sr_{j^1} inside a pair
        double sr[P];
#pragma unroll
        for (int j = 0; j < P; j++) sr[j] = j < PE ? ((j & 1) ? -c.sh[j / 2] : c.sh[j / 2]) : 0.0;
        double rn[P];
#pragma unroll
        for (int j = 0; j < P; j++) rn[j] = (j < PE) ? c.cr[j] * r[j] - sr[j ^ 1] * r[j ^ 1] : c.cr[j] * r[j];
#pragma unroll
        for (int j = 0; j < P; j++) r[j] = rn[j];
        // T = N Phi for j >= i, and below the diagonal the one entry a pair's even row needs from its partner: (i + 1, i)
        double T[P][P];
#pragma unroll
        for (int a = 0; a < P; a++) {
#pragma unroll
            for (int b = 0; b < P; b++) {
                const bool need = (b >= a) || (b == a - 1 && (a & 1) && a < PE);
                if (need) {
                    if (b < PE)
                        T[a][b] = Nm[tri<P>(a, b)] * c.cr[b] - Nm[tri<P>(a, b ^ 1)] * sr[b ^ 1];
                    else
                        T[a][b] = Nm[tri<P>(a, b)] * c.cr[b];
                } else {
                    T[a][b] = 0.0;
                }
            }
        }
#pragma unroll
        for (int a = 0; a < P; a++) {
#pragma unroll
            for (int b = a; b < P; b++) {
                if (a < PE)
                    Nm[tri<P>(a, b)] = c.cr[a] * T[a][b] - sr[a ^ 1] * T[a ^ 1][b];
                else
                    Nm[tri<P>(a, b)] = c.cr[a] * T[a][b];
            }
        }
        c = cp;
    }
}

}  // namespace carma
