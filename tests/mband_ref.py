"""References and the shared case table of the multi-band tests (tests/test_mband_cpu.py, tests/test_gpu_mband.py).

dense_truth   the exact multi-band log-likelihood at 50 digits (mpmath): C_ij = a_i a_j acv(|tau_i - tau_j|) + delta_ij scale
              yerr_i^2, l = -1/2 log det C - 1/2 r^T C^-1 r, tau = t - lag_b, r = y - mu_b; no (N / 2) log 2 pi.  N <= 40.
kalman_ref    a float64 numpy restatement of the merged Kalman filter in complex modal form (as mp_truth.loglik_truth states the
              single-series one), O(N p^2), a batch of parameter vectors at a time: the yardstick where N is too large for
              dense_truth.
Neither contains the log prior of measerr_scale, which every log-density of the library adds: log_prior().
Test code only."""
import functools

import mpmath as mp
import numpy as np

mp.mp.dps = 50


# ---- theta <-> roots ---------------------------------------------------------------------------------------------------------
def log_quads(roots):
    """Log quadratic-factor parameters of roots given as consecutive pairs (a conjugate pair or two real roots) and, for an odd
    count, one real root at the end."""
    roots = [complex(r) for r in roots]
    out = []
    for i in range(len(roots) // 2):
        r1, r2 = roots[2 * i], roots[2 * i + 1]
        out += [np.log((r1 * r2).real), np.log(-(r1 + r2).real)]
    if len(roots) % 2:
        out.append(np.log(-roots[-1].real))
    return out


def make_theta(ysigma, scale, mu, ar_roots, ma_roots=()):
    return np.array([ysigma, scale, mu] + log_quads(ar_roots) + log_quads(ma_roots))


def extend(theta, extras):
    """theta + [(lag_b, a_b, mu_b) for b = 1 ... K - 1] -> the extended vector (log a_b in it)."""
    out = list(theta)
    for lag, a, mu in extras:
        out += [lag, np.log(a), mu]
    return np.array(out, dtype=float)


def log_prior(scale, dof=50.0):
    return -0.5 * dof / scale - (1.0 + dof / 2.0) * np.log(scale)


def _band_params(thx, d, K):
    thx = np.asarray(thx, dtype=float)
    lag, a, mu = [0.0], [1.0], [thx[2]]
    for b in range(1, K):
        c = d + 3 * (b - 1)
        lag.append(thx[c])
        a.append(np.exp(thx[c + 1]))
        mu.append(thx[c + 2])
    return lag, a, mu


# ---- 50 digits ---------------------------------------------------------------------------------------------------------------
def _mp_quad_roots(lq, m):
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


def _mp_acv_terms(th, p, q):
    """[(c_k, w_k)] with acv(lag) = Re sum_k c_k exp(w_k |lag|), from theta at 50 digits (the formulas of mp_truth.loglik_truth)."""
    om = _mp_quad_roots(th[3:3 + p], p)
    ma = [mp.mpf(0)] * p
    if q == 0:
        ma[0] = mp.mpf(1)
    else:
        mr = _mp_quad_roots(th[3 + p:3 + p + q], q)
        cf = [mp.mpc(1)] + [mp.mpc(0)] * q
        for i, r in enumerate(mr):
            for k in range(i + 1, 0, -1):
                cf[k] = cf[k] - r * cf[k - 1]
        pc = [c.real for c in cf]
        for i in range(q + 1):
            ma[i] = pc[q - i] / pc[q]
    terms = []
    for k in range(p):
        dp = mp.mpc(1)
        for l in range(p):
            if l != k:
                dp *= (om[l] - om[k]) * (mp.conj(om[l]) + om[k])
        s1 = sum(ma[l] * om[k] ** l for l in range(p))
        s2 = sum(ma[l] * (-om[k]) ** l for l in range(p))
        terms.append((s1 * s2 / (-2 * om[k].real * dp), om[k]))
    var1 = sum(c for c, _ in terms).real
    sigsqr = th[0] ** 2 / var1
    return [(sigsqr * c, w) for c, w in terms]


def dense_truth(bands, thx, p, q):
    """The exact log-likelihood of the extended vector thx on bands = [(t, y, yerr)] (no prior), as a float."""
    K, d = len(bands), 3 + p + q
    th = [mp.mpf(float(v)) for v in thx]
    terms = _mp_acv_terms(th, p, q)
    tau, r, a, e2 = [], [], [], []
    for b, (t, y, yerr) in enumerate(bands):
        if b == 0:
            lag, ab, mub = mp.mpf(0), mp.mpf(1), th[2]
        else:
            c = d + 3 * (b - 1)
            lag, ab, mub = th[c], mp.exp(th[c + 1]), th[c + 2]
        for ti, yi, ei in zip(t, y, yerr):
            tau.append(mp.mpf(float(ti)) - lag)
            r.append(mp.mpf(float(yi)) - mub)
            a.append(ab)
            e2.append(th[1] * mp.mpf(float(ei)) ** 2)
    N = len(tau)
    assert N <= 40, "dense_truth is meant for N <= 40"
    cache = {}

    def acv(lag):
        if lag not in cache:
            cache[lag] = mp.fsum(c * mp.exp(w * lag) for c, w in terms).real
        return cache[lag]

    C = mp.matrix(N, N)
    for i in range(N):
        for j in range(i + 1):
            v = a[i] * a[j] * acv(abs(tau[i] - tau[j]))
            C[i, j] = v
            C[j, i] = v
        C[i, i] += e2[i]
    L = mp.cholesky(C)
    z = mp.lu_solve(L, mp.matrix(r))                         # (L is triangular: forward substitution by elimination)
    logdet = 2 * mp.fsum(mp.log(L[i, i]) for i in range(N))
    return float(-logdet / 2 - mp.fsum(v * v for v in z) / 2)


# ---- float64 ------------------------------------------------------------------------------------------------------------------
def _np_quad_roots(lq, m):
    roots = []
    for i in range(m // 2):
        q1, q2 = np.exp(lq[2 * i]), np.exp(lq[2 * i + 1])
        disc = q2 * q2 - 4 * q1
        if disc > 0:
            roots += [-(q2 + np.sqrt(disc)) / 2, -(q2 - np.sqrt(disc)) / 2]
        else:
            roots += [complex(-q2 / 2, -np.sqrt(-disc) / 2), complex(-q2 / 2, np.sqrt(-disc) / 2)]
    if m % 2:
        roots.append(-np.exp(lq[m - 1]))
    return np.array(roots, dtype=complex)


def merge_order(bands, lags):
    """(tau, band, index within the band) of the merged series: by shifted time, equal times the lower band first."""
    tau = np.concatenate([np.asarray(t, dtype=float) - lag for (t, _, _), lag in zip(bands, lags)])
    band = np.concatenate([np.full(len(t), b) for b, (t, _, _) in enumerate(bands)])
    idx = np.concatenate([np.arange(len(t)) for t, _, _ in bands])
    o = np.lexsort((band, tau))
    return tau[o], band[o], idx[o]


def _np_model(th, p, q):
    """(om [p], b [p], V [p, p]) of the CARMA part th: AR roots, rotated MA coefficients, stationary covariance."""
    om = _np_quad_roots(th[3:3 + p], p)
    ma = np.zeros(p)
    if q == 0:
        ma[0] = 1.0
    else:
        c = np.real(np.poly(_np_quad_roots(th[3 + p:3 + p + q], q)))           # highest order first
        ma[:q + 1] = (c / c[-1])[::-1]
    E = np.vander(om, p, increasing=True).T                                      # E[i, j] = om_j^i
    b = ma @ E
    var1 = 0.0
    for k in range(p):
        dp = np.prod([(om[l] - om[k]) * (np.conj(om[l]) + om[k]) for l in range(p) if l != k]) if p > 1 else 1.0
        var1 += (np.polyval(ma[::-1], om[k]) * np.polyval(ma[::-1], -om[k]) / (-2.0 * om[k].real * dp)).real
    sigsqr = th[0] ** 2 / var1
    rhs = np.zeros(p, dtype=complex)
    rhs[p - 1] = 1.0
    J = np.linalg.solve(E, rhs)
    V = -sigsqr * np.outer(J, np.conj(J)) / (om[:, None] + np.conj(om)[None, :])
    return om, b, V


def kalman_ref(bands, thx, p, q):
    """The merged Kalman filter in complex modal coordinates, float64 (no prior).  thx: [dx] -> a float, or [B, dx] -> [B]: the
    rows advance together (each on its own merge order), so a batch costs little more than one row."""
    X = np.atleast_2d(np.asarray(thx, dtype=float))
    nb, K, d = X.shape[0], len(bands), 3 + p + q
    N = sum(len(t) for t, _, _ in bands)
    om, b, V = (np.empty((nb, p), dtype=complex), np.empty((nb, p), dtype=complex), np.empty((nb, p, p), dtype=complex))
    tau, yv, av, ev = (np.empty((nb, N)) for _ in range(4))
    yall = np.concatenate([np.asarray(y, dtype=float) for _, y, _ in bands])
    eall = np.concatenate([np.asarray(e, dtype=float) for _, _, e in bands])
    start = np.concatenate([[0], np.cumsum([len(t) for t, _, _ in bands])])
    for r in range(nb):
        om[r], b[r], V[r] = _np_model(X[r], p, q)
        lag, a, mu = _band_params(X[r], d, K)
        tau[r], band, idx = merge_order(bands, lag)
        src = start[band] + idx
        yv[r] = yall[src] - np.asarray(mu)[band]
        av[r] = np.asarray(a)[band]
        ev[r] = X[r, 1] * eall[src] ** 2
    bc = np.conj(b)
    x = np.zeros((nb, p), dtype=complex)
    P = V.copy()
    ll = np.zeros(nb)
    for s in range(N):
        if s:
            rho = np.exp(om * (tau[:, s] - tau[:, s - 1])[:, None])
            x = rho * x
            P = rho[:, :, None] * np.conj(rho)[:, None, :] * (P - V) + V
        Pb = np.einsum("rij,rj->ri", P, bc)
        var = av[:, s] ** 2 * np.einsum("ri,ri->r", b, Pb).real + ev[:, s]
        innov = yv[:, s] - av[:, s] * np.einsum("ri,ri->r", b, x).real
        ll += -0.5 * np.log(var) - 0.5 * innov * innov / var
        g = av[:, s, None] * Pb / var[:, None]
        x = x + g * innov[:, None]
        P = P - var[:, None, None] * g[:, :, None] * np.conj(g)[:, None, :]
    return float(ll[0]) if np.ndim(thx) == 1 else ll


def neg_logpost_and_grad(bands, p, q, fd_step=1e-6):
    """x -> (f, g) for scipy's L-BFGS-B: f = -(kalman_ref + log_prior(measerr_scale)), g by central differences of relative step
    fd_step (the stencil of the library's optimiser), all 2 dx + 1 points in one kalman_ref batch."""
    def fg(x):
        x = np.asarray(x, dtype=float)
        n = x.size
        h = fd_step * np.maximum(1.0, np.abs(x))
        pts = np.tile(x, (2 * n + 1, 1))
        pts[1:n + 1] += np.diag(h)
        pts[n + 1:] -= np.diag(h)
        with np.errstate(all="ignore"):
            f = -(kalman_ref(bands, pts, p, q) + log_prior(pts[:, 1]))
        ok = np.isfinite(f[1:n + 1]) & np.isfinite(f[n + 1:])
        g = np.where(ok, (f[1:n + 1] - f[n + 1:]) / (2.0 * h), 0.0)
        return (f[0] if np.isfinite(f[0]) else 1e300), g
    return fg


# ---- the case table -----------------------------------------------------------------------------------------------------------
ORDERS = [(1, 0), (2, 1), (3, 0), (4, 2), (5, 3), (7, 6)]

# per order: two root sets (pairs are consecutive entries), the second with a quadratic factor of two REAL roots where p >= 2
_AR = {
    1: [[-0.5], [-0.9]],              # (inside the CAR(1) bounds of every scenario's band 0, which ignore_prior does not lift)
    2: [[-0.2 - 0.7j, -0.2 + 0.7j], [-0.6, -0.15]],
    3: [[-0.15 - 0.8j, -0.15 + 0.8j, -0.4], [-0.5, -0.1, -1.2]],
    4: [[-0.2 - 1.0j, -0.2 + 1.0j, -0.1 - 0.4j, -0.1 + 0.4j], [-0.25 - 0.9j, -0.25 + 0.9j, -0.55, -0.12]],
    5: [[-0.2 - 1.1j, -0.2 + 1.1j, -0.1 - 0.45j, -0.1 + 0.45j, -0.6], [-0.3 - 0.9j, -0.3 + 0.9j, -0.45, -0.1, -1.3]],
    7: [[-0.25 - 1.3j, -0.25 + 1.3j, -0.15 - 0.7j, -0.15 + 0.7j, -0.08 - 0.3j, -0.08 + 0.3j, -0.5],
        [-0.3 - 1.2j, -0.3 + 1.2j, -0.12 - 0.5j, -0.12 + 0.5j, -0.35, -0.07, -0.9]],
}
_MA = {0: [], 1: [-1.5], 2: [-2.5, -0.8], 3: [-2.5, -0.8, -1.6], 6: [-2.0, -0.7, -1.0 - 0.6j, -1.0 + 0.6j, -3.0, -1.4]}


def order_thetas(p, q):
    """The two CARMA parts of order (p, q)."""
    return [make_theta(1.3, 1.1, 0.4, _AR[p][0], _MA[q]), make_theta(0.9, 0.9, -0.2, _AR[p][1], _MA[q])]


def _band(rng, n, t0=0.0, level=0.0, amp=1.0):
    """n data at times on a grid of 1/4 (sums and differences of such times, and of lags on that grid, are exact)."""
    t = t0 + 0.25 * np.cumsum(rng.integers(1, 8, n))
    return t, level + amp * rng.standard_normal(n), amp * rng.uniform(0.1, 0.3, n)


def scenario(name, seed=0):
    """(bands, extras): extras = [(lag_b, a_b, mu_b)] for b >= 1.  All on a time grid of 1/4."""
    rng = np.random.default_rng(1000 + seed)
    if name == "one_band":
        return [_band(rng, 14)], []
    b0 = _band(rng, 12)
    if name == "lag0_shared_stamps":                         # band 1 observes at 8 of band 0's own times: ties at lag 0
        pick = np.sort(rng.choice(12, 8, replace=False))
        return [b0, (b0[0][pick], 3.0 + 2.0 * rng.standard_normal(8), rng.uniform(0.2, 0.5, 8))], [(0.0, 2.0, 3.0)]
    if name == "lag_equals_offset":                          # band 1's times are band 0's + 2.5 and the lag is 2.5: ties
        return [b0, (b0[0][2:11] + 2.5, 1.0 + 0.5 * rng.standard_normal(9), rng.uniform(0.05, 0.15, 9))], [(2.5, 0.5, 1.0)]
    if name == "band1_first":                                # every datum of band 1 ahead of band 0's first
        return [b0, _band(rng, 9, t0=1.0, level=-1.0, amp=1.5)], [(20.0, 1.5, -1.0)]
    if name == "disjoint_after":                             # ... and behind band 0's last
        return [b0, _band(rng, 9, t0=0.5, level=2.0, amp=0.7)], [(-30.25, 0.7, 2.0)]
    if name == "three_bands_7_1_12":
        return ([_band(rng, 7), _band(rng, 1, t0=2.0, level=1.0), _band(rng, 12, t0=-1.0, level=-2.0, amp=3.0)],
                [(1.125, 0.8, 1.0), (-0.6875, 3.0, -2.0)])
    if name == "eight_bands":                                # 2 ... 5 data each; bands 3 and 6 land on band 0's grid (ties)
        ns = [5, 2, 3, 4, 2, 5, 3, 4]
        bands = [_band(rng, n, t0=0.5 * k, level=0.3 * k, amp=1.0 + 0.2 * k) for k, n in enumerate(ns)]
        extras = [(0.3 * k - 1.0, 1.0 + 0.2 * k, 0.3 * k) for k in range(1, 8)]
        extras[2] = (0.5, 1.6, 0.9)
        extras[5] = (-0.25, 2.2, 1.8)
        return bands, extras
    raise KeyError(name)


SCENARIOS = ["one_band", "lag0_shared_stamps", "lag_equals_offset", "band1_first", "disjoint_after", "three_bands_7_1_12",
             "eight_bands"]
CASES = [(p, q, s) for p, q in ORDERS for s in SCENARIOS]


@functools.lru_cache(None)
def case(p, q, name):
    """(bands, thx [2, dx], dense_truth [2]) of a case: computed once per process, shared by the tests that need it."""
    bands, extras = scenario(name, seed=p)
    thx = np.array([extend(th, extras) for th in order_thetas(p, q)])
    truth = np.array([dense_truth(bands, x, p, q) for x in thx])
    return bands, thx, truth


def flat(bands):
    """(time, y, yerr, offsets) as the C ABI takes the bands."""
    off = np.zeros(len(bands) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(b[0]) for b in bands])
    return tuple(np.ascontiguousarray(np.concatenate([np.asarray(b[k], dtype=float) for b in bands])) for k in range(3)) + (off,)


# ---- the lag-recovery problem ---------------------------------------------------------------------------------------------------
RECOVERY_SEED = 3
RECOVERY_LAGS = np.arange(9.0)                               # the true lag 4.0 is on the grid
RECOVERY_TRUE_LAG = 4.0


@functools.lru_cache(None)
def recovery_problem(seed=RECOVERY_SEED):
    """Two bands of 60 data of one CARMA(2,1) path (carma_process on the host): band 1 = 2 x(t - 4) + 0.5, noise 1 % of the
    process' standard deviation.  Returns (bands, the extended vector the data were drawn from)."""
    from carma_pack_amd.carma_pack import carma_process, carma_variance
    rng = np.random.default_rng(seed)
    ar, ma_roots = np.array([-0.05 - 0.2j, -0.05 + 0.2j]), [-0.5]
    ma = np.array([1.0, 2.0])                                # 1 + s / 0.5
    sigma, a, mu0, mu1, lag = 1.0, 2.0, 10.0, 0.5, RECOVERY_TRUE_LAG
    t0 = np.cumsum(rng.uniform(1.0, 3.0, 60))
    t1 = np.cumsum(rng.uniform(1.0, 3.0, 60)) + 2.0
    tt = np.concatenate([t0, t1 - lag])
    o = np.argsort(tt, kind="stable")
    x = np.empty(120)
    x[o] = carma_process(tt[o], sigma ** 2 / carma_variance(1.0, ar, ma), ar, ma_coefs=ma, rng=rng)
    e0, e1 = np.full(60, 0.01 * sigma), np.full(60, 0.01 * sigma * a)
    bands = [(t0, mu0 + x[:60] + e0 * rng.standard_normal(60), e0), (t1, mu1 + a * x[60:] + e1 * rng.standard_normal(60), e1)]
    return bands, extend(make_theta(sigma, 1.0, mu0, ar, ma_roots), [(lag, a, mu1)])


def recovery_box(bands, p=2, q=1):
    """(lo, hi) [dx] of the optimisers on the recovery problem: CarmaModel._mle_bounds on band 0, the band parameters free."""
    from carma_pack_amd.carma_pack import CarmaModel
    t, y, e = bands[0]
    b = CarmaModel.__new__(CarmaModel)
    b.time, b.y = t, y
    bn = b._mle_bounds(p, q)
    lo = np.array([-np.inf if v[0] is None else v[0] for v in bn] + [-np.inf] * 3)
    hi = np.array([np.inf if v[1] is None else v[1] for v in bn] + [np.inf] * 3)
    return lo, hi


def kalman_profile(bands, x_start, lags, p=2, q=1):
    """The profile log-likelihood of kalman_ref over the lag of band 1 (two bands): scipy's L-BFGS-B on the other variables from
    x_start at each lag.  Returns [L]."""
    from scipy.optimize import minimize
    d = 3 + p + q
    lo, hi = recovery_box(bands, p, q)
    free = [j for j in range(d + 3) if j != d]
    out = []
    for lag in lags:
        fg = neg_logpost_and_grad(bands, p, q)

        def f(z, lag=lag, fg=fg):
            x = np.empty(d + 3)
            x[free] = z
            x[d] = lag
            v, g = fg(x)
            return v, g[free]

        r = minimize(f, np.asarray(x_start)[free], jac=True, method="L-BFGS-B", bounds=list(zip(lo[free], hi[free])))
        out.append(-r.fun)
    return np.array(out)
