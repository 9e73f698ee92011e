// carma_smooth.h -- the fixed-interval smoother in ONE forward and ONE backward pass over the series: the interpolated light
// curve (mean and variance of the noise-free process given ALL the data) at M times for O((n + M) p^2), where a predict_run
// per time (carma_predict.h) costs O(M n p^2).  Included by carma_smooth.hip (gfx950) and tests/emu/emu_smooth.cpp (CPU lane
// emulator, test harness only).
//
// Modified Bryson-Frazier form on the recursion of carma_core.h (rotated basis, D = P - V, row r of a matrix in lane r).  The
// grid has ng = n + M points in ascending time; point i is a datum (src[i] = j >= 0) or a requested time (src[i] = -1 - i').
//
// Forward (the arithmetic of predict_run's "before" branch), at point i with the PREDICTED state x_i, D_i:
//     u_i = P_i b^H = D_i b^H + c        f_i = Re(b P_i b^H) = s0 + Re(b D_i b^H)        Sx_i = Re(b x_i)
//   datum:  F_i = f_i + yerr^2,  v_i = (y - mu) - Sx_i,  x += u v / F,  D -= u u^H / F
//   then the transition to point i + 1:  x <- rho o x,  D <- rho rho^H o D,  rho = exp(omega dt)
//   and the record {u_i, rho_i} of every lane and {1/F_i (0 at a requested time), v_i, Sx_i, f_i} of the group are stored.
// Backward, from r = 0, N = 0 (N Hermitian) at the last point down to the first:
//     r <- conj(rho_i) o r,   N_jk <- conj(rho_ij) rho_ik N_jk           (the step from point i + 1 back to point i)
//     a = N u_i,   qn = u_i^H a,   h = u_i^H r                           (both real: the root set is closed under conjugation)
//   requested time:  mean = Sx_i + h (+ mu),   var = f_i - qn
//   datum, K = u_i / F_i, L = I - K b:
//     r <- b^H v_i / F_i + L^H r = r + b^H (v_i - h) / F_i
//     N <- b^H b / F_i + L^H N L = N_jk - (a_j / F) b_k - conj(b_j) conj(a_k / F) + conj(b_j) b_k (qn / F^2 + 1 / F)
// Two exchanges ({u, rho} and a / F) and two group sums per backward step.  A forecast or backcast needs no special case:
// behind the last datum r = N = 0, before the first one the backward pass has collected every datum.
//
// The variance is the difference f - u^H N u and is returned AS COMPUTED: it loses log10(f / var) digits, like the D = P - V
// filter behind predict_run, and where the data pin the process far below its prior variance (yerr << sd) it may come out
// <= 0 by rounding.  Nothing is clipped.
#pragma once
#include "carma_core.h"
#include "carma_predict.h"

namespace carma {

// rec / grp: this lane's record and this group's record of point 0; rs / gs: their strides from point to point (double4 units).
// Lane 0 of the group stores the group record; the caller separates the two passes by a barrier that makes it visible.
template <int P, int G, class GrpT>
CARMA_DEV void smooth_forward(const GrpT& g, const Model<P>& m, const FilterConsts<P>& fc, const double4* __restrict__ series,
                              const double* __restrict__ grid, const int* __restrict__ src, int ng, double mu,
                              double4* __restrict__ rec, long rs, double4* __restrict__ grp, long gs)
{
    const Cx b = fc.b_msk, c_own = fc.c_own;
    const double s0 = fc.s0;
    Cx ball[P];
#pragma unroll
    for (int j = 0; j < P; j++) ball[j] = fc.ball[j];
    Cx D[P];
#pragma unroll
    for (int j = 0; j < P; j++) D[j] = {0.0, 0.0};
    Cx x = {0.0, 0.0};
    Cx u = c_own;
    double f = s0, Sx = 0.0;
    const bool lane0 = g.lane() == 0;
    // what the next point needs from memory is fetched a step ahead: the loads are off the recursion's dependent chain
    int si = src[0];
    double4 r = series[si >= 0 ? si : 0];
    double t_i = grid[0];
    for (int i = 0; i < ng; i++) {
        const int in = (i + 1 < ng) ? i + 1 : i;
        const int si_n = src[in];
        const double4 r_n = series[si_n >= 0 ? si_n : 0];
        const double t_n = grid[in];
        double s = 0.0, v = 0.0;
        if (si >= 0) {                                        // (wave-uniform: every model of a launch walks the same grid)
            v = (r.y - mu) - Sx;
            s = 1.0 / (f + r.z);
        }
        const double dt = t_n - t_i;                          // (the last point: 0)
        Cx rho;
        cexp_step(m.w.re, m.w.im, dt, &rho.re, &rho.im);
        rec[(long)i * rs] = make_double4(u.re, u.im, rho.re, rho.im);
        if (lane0) grp[(long)i * gs] = make_double4(s, v, Sx, f);
        // measurement update (s = 0: none) and transition, as predict_run
        const Cx gk = {u.re * s, u.im * s};
        x = {x.re + gk.re * v, x.im + gk.im * v};
        g.publish(u.re, u.im, rho.re, rho.im);
        Cx w = {0.0, 0.0};
#pragma unroll
        for (int j = 0; j < P; j++) {
            const double4 o = g.peek(j);
            const Cx t = cmulc(u, Cx{o.x, o.y});
            const Cx d = {fma(-t.re, s, D[j].re), fma(-t.im, s, D[j].im)};
            D[j] = cmul(cmulc(rho, Cx{o.z, o.w}), d);
            w = cadd(w, cmulc(D[j], ball[j]));
        }
        g.done_reading();
        u = cadd(w, c_own);
        x = cmul(rho, x);
        f = s0 + g.sum(b.re * w.re - b.im * w.im);
        Sx = g.sum(b.re * x.re - b.im * x.im);
        si = si_n;
        r = r_n;
        t_i = t_n;
    }
}

// pmean / pvar: the model's M outputs in the caller's order, or null (a group that only keeps its wave's loop uniform)
template <int P, int G, class GrpT>
CARMA_DEV void smooth_backward(const GrpT& g, const FilterConsts<P>& fc, const int* __restrict__ src, int ng, double mu,
                               const double4* __restrict__ rec, long rs, const double4* __restrict__ grp, long gs,
                               double* __restrict__ pmean, double* __restrict__ pvar)
{
    const bool act = g.lane() < P;
    const bool lane0 = g.lane() == 0;
    const Cx bo = fc.b_own;
    Cx ball[P];
#pragma unroll
    for (int j = 0; j < P; j++) ball[j] = fc.ball[j];
    Cx N[P];
#pragma unroll
    for (int j = 0; j < P; j++) N[j] = {0.0, 0.0};
    Cx r = {0.0, 0.0};
    // the records of point i - 1 are loaded while point i is worked on (their latency would sit on the dependent chain)
    double4 q = rec[(long)(ng - 1) * rs];
    double4 c = grp[(long)(ng - 1) * gs];
    int si = src[ng - 1];
    for (int i = ng - 1; i >= 0; i--) {
        const int ip = i > 0 ? i - 1 : 0;
        const double4 q_p = rec[(long)ip * rs];
        const double4 c_p = grp[(long)ip * gs];
        const int si_p = src[ip];
        const Cx u = {q.x, q.y}, rhoc = {q.z, -q.w};          // conj(rho_i); the last point's rho is 1
        const double s = c.x, v = c.y;
        g.publish(q.x, q.y, q.z, q.w);
        Cx a = {0.0, 0.0};
#pragma unroll
        for (int j = 0; j < P; j++) {
            const double4 o = g.peek(j);
            N[j] = cmul(cmul(rhoc, Cx{o.z, o.w}), N[j]);
            a = cadd(a, cmul(N[j], Cx{o.x, o.y}));
        }
        g.done_reading();
        r = cmul(rhoc, r);
        const double qn = g.sum(act ? u.re * a.re + u.im * a.im : 0.0);
        const double h = g.sum(act ? u.re * r.re + u.im * r.im : 0.0);
        if (si < 0) {
            if (pmean && lane0) {
                pmean[-1 - si] = add_back_mu(c.z + h, mu);
                pvar[-1 - si] = c.w - qn;
            }
        } else {
            const Cx ak = {a.re * s, a.im * s};
            const double coef = fma(qn * s, s, s);
            const double gr = s * (v - h);
            r = {fma(bo.re, gr, r.re), fma(-bo.im, gr, r.im)};
            g.publish2(ak.re, ak.im);
            const Cx bc = {bo.re * coef, -bo.im * coef};     // conj(b_j) (qn / F^2 + 1 / F)
#pragma unroll
            for (int k = 0; k < P; k++) {
                const Cx ao = g.peek2(k);
                const Cx t1 = cmul(ak, ball[k]);              // (a_j / F) b_k
                const Cx t2 = cmulc(Cx{bo.re, -bo.im}, ao);   // conj(b_j) conj(a_k / F)
                const Cx t3 = cmul(bc, ball[k]);
                N[k] = {N[k].re - t1.re - t2.re + t3.re, N[k].im - t1.im - t2.im + t3.im};
            }
            g.done_reading();
        }
        q = q_p;
        c = c_p;
        si = si_p;
    }
}

// CAR(1): every quantity a scalar, one lane per model.  sc: this lane's slot of plane 0, point 0; ps: stride from point to
// point, qs: from plane to plane ({phi, 1/F or 0, v, x, f}).
CARMA_DEV void smooth_car1(double sigsqr, double omega, double mu, const double4* __restrict__ series,
                           const double* __restrict__ grid, const int* __restrict__ src, int ng, double* __restrict__ sc, long ps,
                           long qs, double* __restrict__ pmean, double* __restrict__ pvar)
{
    const double sv = sigsqr / (2.0 * omega);
    double x = 0.0, pv = sv;
    for (int i = 0; i < ng; i++) {
        const int si = src[i];
        const double f = pv, sx = x;
        double s = 0.0, v = 0.0;
        if (si >= 0) {
            const double4 rc = series[si];
            s = 1.0 / (f + rc.z);
            v = (rc.y - mu) - x;
            x = fma(f * s, v, x);
            pv = f * (rc.z * s);                              // f (1 - k), k = f / F: no cancellation
        }
        const double phi = (i + 1 < ng) ? exp(-omega * (grid[i + 1] - grid[i])) : 1.0;
        x *= phi;
        pv = sv * (1.0 - phi * phi) + phi * phi * pv;
        double* o = sc + (long)i * ps;
        o[0] = phi;
        o[qs] = s;
        o[2 * qs] = v;
        o[3 * qs] = sx;
        o[4 * qs] = f;
    }
    double r = 0.0, N = 0.0;
    // (point i - 1 is loaded while point i is worked on, as in smooth_backward)
    const double* o = sc + (long)(ng - 1) * ps;
    double phi = o[0], s = o[qs], v = o[2 * qs], sx = o[3 * qs], f = o[4 * qs];
    int si = src[ng - 1];
    double e2 = series[si >= 0 ? si : 0].z;
    for (int i = ng - 1; i >= 0; i--) {
        const int ip = i > 0 ? i - 1 : 0;
        const double* op = sc + (long)ip * ps;
        const double phi_p = op[0], s_p = op[qs], v_p = op[2 * qs], sx_p = op[3 * qs], f_p = op[4 * qs];
        const int si_p = src[ip];
        const double e2_p = series[si_p >= 0 ? si_p : 0].z;
        r *= phi;
        N *= phi * phi;
        if (si < 0) {
            if (pmean) {
                pmean[-1 - si] = add_back_mu(fma(f, r, sx), mu);
                pvar[-1 - si] = fma(-(f * f), N, f);
            }
        } else {
            const double omk = e2 * s;                        // 1 - k
            r = fma(omk, r, v * s);
            N = fma(omk * omk, N, s);
        }
        phi = phi_p;
        s = s_p;
        v = v_p;
        sx = sx_p;
        f = f_p;
        si = si_p;
        e2 = e2_p;
    }
}

}  // namespace carma
