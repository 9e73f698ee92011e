"""High-precision (mpmath, 50 digits) evaluation of the reference's log-likelihood recursion, used
only to arbitrate ill-conditioned cases: where cond(EigenMat) >~ 1e6 two double-precision
implementations of kfilter.cpp (the reference's LAPACK path, the oracle's LU, the GPU's lane-
distributed LU) legitimately differ by more than 1e-10, and the question becomes which one is
closer to the exact value.  Literal restatement of kfilter.cpp:138-215 + carpack.hpp:167-171."""
import mpmath as mp
import numpy as np

mp.mp.dps = 50


def loglik_truth(t, y, yerr, theta, p, q):
    th = [mp.mpf(float(v)) for v in theta]

    def quad_roots(lq, m):
        roots = []
        for i in range(m // 2):
            q1, q2 = mp.exp(lq[2 * i]), mp.exp(lq[2 * i + 1])
            disc = q2 * q2 - 4 * q1
            if disc > 0:
                roots += [-(q2 + mp.sqrt(disc)) / 2, -(q2 - mp.sqrt(disc)) / 2]
            else:
                roots += [mp.mpc(-q2 / 2, -mp.sqrt(-disc) / 2), mp.mpc(-q2 / 2, mp.sqrt(-disc) / 2)]
        if m % 2:
            roots.append(-mp.exp(lq[m - 1]))
        return [mp.mpc(r) for r in roots]

    om = quad_roots(th[3:3 + p], p)
    ma = [mp.mpf(0)] * p
    if q == 0:
        ma[0] = mp.mpf(1)
    else:
        mr = quad_roots(th[3 + p:3 + p + q], q)
        cf = [mp.mpc(1)] + [mp.mpc(0)] * q
        for i, r in enumerate(mr):
            for k in range(i + 1, 0, -1):
                cf[k] = cf[k] - r * cf[k - 1]
        pc = [c.real for c in cf]
        for i in range(q + 1):
            ma[i] = pc[q - i] / pc[q]
    # Variance(omega, ma, 1)
    var1 = mp.mpc(0)
    for k in range(p):
        dp = mp.mpc(1)
        for l in range(p):
            if l != k:
                dp *= (om[l] - om[k]) * (mp.conj(om[l]) + om[k])
        den = -2 * om[k].real * dp
        s1 = sum(ma[l] * om[k] ** l for l in range(p))
        s2 = sum(ma[l] * (-om[k]) ** l for l in range(p))
        var1 += s1 * s2 / den
    sigsqr = th[0] ** 2 / var1.real
    scale, mu = th[1], th[2]
    E = mp.matrix(p, p)
    for i in range(p):
        for j in range(p):
            E[i, j] = om[j] ** i
    rhs = mp.matrix(p, 1)
    rhs[p - 1] = 1
    J = mp.lu_solve(E, rhs)
    b = [sum(ma[i] * E[i, j] for i in range(p)) for j in range(p)]
    V = [[-sigsqr * J[i] * mp.conj(J[j]) / (om[i] + mp.conj(om[j])) for j in range(p)] for i in range(p)]
    P = [row[:] for row in V]
    x = [mp.mpc(0)] * p
    tt = [mp.mpf(float(v)) for v in t]
    yy = [mp.mpf(float(v)) - mu for v in y]
    ee = [scale * mp.mpf(float(v)) ** 2 for v in yerr]
    var = sum(b[i] * sum(P[i][j] * mp.conj(b[j]) for j in range(p)) for i in range(p)).real + ee[0]
    mean = mp.mpf(0)
    innov = yy[0]
    ll = -mp.log(var) / 2 - innov ** 2 / var / 2
    for k in range(1, len(tt)):
        g = [sum(P[i][j] * mp.conj(b[j]) for j in range(p)) / var for i in range(p)]
        x = [x[i] + g[i] * innov for i in range(p)]
        P = [[P[i][j] - var * g[i] * mp.conj(g[j]) for j in range(p)] for i in range(p)]
        dt = tt[k] - tt[k - 1]
        rho = [mp.exp(om[i] * dt) for i in range(p)]
        x = [rho[i] * x[i] for i in range(p)]
        P = [[rho[i] * mp.conj(rho[j]) * (P[i][j] - V[i][j]) + V[i][j] for j in range(p)] for i in range(p)]
        mean = sum(b[i] * x[i] for i in range(p)).real
        var = sum(b[i] * sum(P[i][j] * mp.conj(b[j]) for j in range(p)) for i in range(p)).real + ee[k]
        innov = yy[k] - mean
        ll += -mp.log(var) / 2 - innov ** 2 / var / 2
    logprior = -mp.mpf(50) / 2 / scale - 26 * mp.log(scale)
    return float(ll + logprior), float(ll)


def _acv_terms_carma(sigsqr, roots, ma):
    """The autocovariance of the CARMA process as acv(lag) = Re sum_k c_k exp(w_k |lag|): the sum over the AR roots that
    oracle.variance (carpack.cpp:377-409) evaluates, here at 50 digits from the double inputs.  Returns [(c_k, w_k)]."""
    om = [mp.mpc(complex(r)) for r in roots]
    p = len(om)
    beta = [mp.mpf(float(v)) for v in ma] + [mp.mpf(0)] * (p - len(ma))
    terms = []
    for k in range(p):
        dp = mp.mpc(1)
        for l in range(p):
            if l != k:
                dp *= (om[l] - om[k]) * (mp.conj(om[l]) + om[k])
        s1 = sum(beta[l] * om[k] ** l for l in range(p))
        s2 = sum(beta[l] * (-om[k]) ** l for l in range(p))
        terms.append((mp.mpf(float(sigsqr)) * s1 * s2 / (-2 * om[k].real * dp), om[k]))
    return terms


def _dense_conditional(terms, t, y, yerr, tpred):
    """E, Var of the process at each of tpred given the data, acv(lag) = Re sum_k c_k exp(w_k |lag|).
    exp(w (t_i - t_j)) = exp(w t_i) exp(-w t_j): n exponentials per root instead of n^2 / 2.  The covariances are mp values
    (50 digits); the linear algebra runs on them as integers in units of 2^-256 (exact products and sums, one rounding per
    division or square root): the same digits as mp matrices, ~20x faster, so a 270-point series takes about a second."""
    from math import isqrt
    from operator import mul
    F = 256
    fix = lambda v: int(mp.nint(mp.ldexp(v, F)))                                 # noqa: E731
    dot = lambda a, b: sum(map(mul, a, b)) >> F                                 # noqa: E731
    tt = [mp.mpf(float(v)) for v in t]
    n = len(tt)
    # row i: the 2p reals (Re, -Im) of c_k exp(w_k t_i); column j: (Re, Im) of exp(-w_k t_j); K_ij = their dot product
    up, dn = [], []
    for ti in tt:
        a = [c * mp.exp(w * ti) for c, w in terms]
        b = [mp.exp(-w * ti) for c, w in terms]
        up.append([v.real for v in a] + [-v.imag for v in a])
        dn.append([v.real for v in b] + [v.imag for v in b])

    def acv(lag):
        return mp.fsum(c * mp.exp(w * lag) for c, w in terms).real

    def kdd(i, j):
        return fix(mp.fdot(up[i], dn[j]) if tt[i] >= tt[j] else mp.fdot(up[j], dn[i]))

    # K_dd + diag(yerr^2), Cholesky-factored once
    L = [[0] * n for _ in range(n)]
    for j in range(n):
        Lj = L[j]
        Lj[j] = isqrt((fix(acv(mp.mpf(0)) + mp.mpf(float(yerr[j])) ** 2) - dot(Lj[:j], Lj[:j])) << F)
        for i in range(j + 1, n):
            Li = L[i]
            Li[j] = ((kdd(i, j) << F) - sum(map(mul, Li[:j], Lj[:j]))) // Lj[j]

    def lsolve(v):
        z = []
        for i in range(n):
            z.append(((v[i] << F) - sum(map(mul, L[i][:i], z))) // L[i][i])
        return z

    a = lsolve([fix(mp.mpf(float(v))) for v in y])
    k0 = fix(acv(mp.mpf(0)))
    mean, var = np.empty(len(tpred)), np.empty(len(tpred))
    for m, tp in enumerate(tpred):
        tp = mp.mpf(float(tp))
        b = lsolve([fix(acv(abs(tp - ti))) for ti in tt])
        mean[m] = float(mp.ldexp(dot(a, b), -F))
        var[m] = float(mp.ldexp(k0 - dot(b, b), -F))
    return mean, var


def predict_truth(t, y, yerr, sigsqr, roots, ma, tpred):
    """KalmanFilterp::Predict (kfilter.cpp:218-337) at 50 digits, as what it computes: the dense Gaussian-process
    conditional of the process at each of `tpred` given the data, E = k' C^-1 y, Var = acv(0) - k' C^-1 k with
    C = K_dd + diag(yerr^2), factored once for all times.  y centred and yerr already scaled, as for
    oracle.predict_carma; the series is used as given (sort_dedup it first to mirror the filter).  Meant for series of
    <= 80 points (cost O(n^2 p) mp operations + O(n^3) integer ones)."""
    return _dense_conditional(_acv_terms_carma(sigsqr, roots, ma), t, y, yerr, tpred)


def predict_truth_car1(t, y, yerr, sigsqr, omega, tpred):
    """predict_truth of a CAR(1) process (KalmanFilter1::Predict, kfilter.cpp:72-135): acv(lag) = sigsqr / (2 omega)
    exp(-omega |lag|)."""
    return _dense_conditional([(mp.mpf(float(sigsqr)) / (2 * mp.mpf(float(omega))), -mp.mpf(float(omega)))],
                              t, y, yerr, tpred)
