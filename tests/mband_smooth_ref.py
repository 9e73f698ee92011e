"""References and the shared table of the multi-band smoother tests (tests/test_mband_smooth_cpu.py, tests/test_gpu_mband_smooth.py).

dense_smooth_truth  the exact Gaussian-process conditional mean and variance of a_b x(tout - lag_b) + mu_b given all data, at 50
                    digits (mpmath), from the covariance mband_ref.dense_truth builds.  N <= 40.
kalman_smooth_ref   a float64 numpy forward / backward (modified Bryson-Frazier) smoother in complex modal form over the merged
                    order, a batch of parameter vectors at a time: the yardstick where N is too large for dense_smooth_truth.
requested_times     the M = 12 requested times of a case of mband_ref.CASES.
Test code only."""
import functools

import mpmath as mp
import numpy as np

import mband_ref as R

RTOL = 1e-9                                                   # the project's smoother rule (tests/test_gpu_smooth.py)


# ---- 50 digits ---------------------------------------------------------------------------------------------------------------
def _fwd_subst(L, b):
    n = len(b)
    z = [mp.mpf(0)] * n
    for i in range(n):
        z[i] = (b[i] - mp.fsum(L[i, j] * z[j] for j in range(i))) / L[i, i]
    return z


def _dense_factor(bands, thx, p, q):
    """What every requested time shares: the acv terms, the shifted times, the band scales, the Cholesky factor of the data
    covariance (as dense_truth builds it) and L^-1 r."""
    K, d = len(bands), 3 + p + q
    th = [mp.mpf(float(v)) for v in thx]
    terms = R._mp_acv_terms(th, p, q)
    par = [(mp.mpf(0), mp.mpf(1), th[2])] + [(th[d + 3 * (b - 1)], mp.exp(th[d + 3 * (b - 1) + 1]), th[d + 3 * (b - 1) + 2])
                                             for b in range(1, K)]
    tau, r, a, e2 = [], [], [], []
    for b, (t, y, yerr) in enumerate(bands):
        lag, ab, mub = par[b]
        for ti, yi, ei in zip(t, y, yerr):
            tau.append(mp.mpf(float(ti)) - lag)
            r.append(mp.mpf(float(yi)) - mub)
            a.append(ab)
            e2.append(th[1] * mp.mpf(float(ei)) ** 2)
    N = len(tau)
    assert N <= 40, "dense_smooth_truth is meant for N <= 40"

    def acv(lag):
        return mp.fsum(c * mp.exp(w * lag) for c, w in terms).real

    C = mp.matrix(N, N)
    for i in range(N):
        for j in range(i + 1):
            v = a[i] * a[j] * acv(abs(tau[i] - tau[j]))
            C[i, j] = v
            C[j, i] = v
        C[i, i] += e2[i]
    L = mp.cholesky(C)
    return par, acv, tau, a, L, _fwd_subst(L, r)


_factor_cache = {}


def dense_smooth_truth(bands, thx, p, q, band, tout):
    """(mean [M], var [M]) of a_b x(tout - lag_b) + mu_b given all data of bands = [(t, y, yerr)] under the extended vector thx:
    mean = mu_b + c^T C^-1 r, var = a_b^2 acv(0) - c^T C^-1 c, c_i = a_b a_i acv(|tout - lag_b - tau_i|).  Floats."""
    key = (id(bands), np.asarray(thx, dtype=float).tobytes(), p, q)
    if key not in _factor_cache:
        _factor_cache[key] = (bands, _dense_factor(bands, thx, p, q))          # (bands kept alive: its id is the key)
    par, acv, tau, a, L, z = _factor_cache[key][1]
    lag, ab, mub = par[band]
    mean, var = [], []
    for to in np.atleast_1d(np.asarray(tout, dtype=float)):
        ts = mp.mpf(float(to)) - lag
        c = [ab * a[i] * acv(abs(ts - tau[i])) for i in range(len(tau))]
        w = _fwd_subst(L, c)
        mean.append(float(mub + mp.fsum(wi * zi for wi, zi in zip(w, z))))
        var.append(float(ab * ab * acv(mp.mpf(0)) - mp.fsum(wi * wi for wi in w)))
    return np.array(mean), np.array(var)


# ---- float64 ------------------------------------------------------------------------------------------------------------------
def kalman_smooth_ref(bands, thx, p, q, band, tout):
    """The merged forward filter of mband_ref.kalman_ref with the requested times of band `band` as one more stream (index K: a
    requested time equal to a datum's shifted time comes behind it), then the adjoint recursion back over the stored records.
    thx: [dx] -> (mean [M], var [M]), or [B, dx] -> ([B, M], [B, M]): the rows advance together, each on its own merge order."""
    X = np.atleast_2d(np.asarray(thx, dtype=float))
    tout = np.atleast_1d(np.asarray(tout, dtype=float))
    nb, K, d, M = X.shape[0], len(bands), 3 + p + q, tout.size
    N = sum(len(t) for t, _, _ in bands)
    ng = N + M
    om, b, V = (np.empty((nb, p), dtype=complex), np.empty((nb, p), dtype=complex), np.empty((nb, p, p), dtype=complex))
    tau, yv, av, ev = (np.empty((nb, ng)) for _ in range(4))
    slot = np.empty((nb, ng), dtype=int)                     # -1: a datum
    ao, muo = np.empty(nb), np.empty(nb)
    tall = np.concatenate([np.asarray(t, dtype=float) for t, _, _ in bands])
    yall = np.concatenate([np.asarray(y, dtype=float) for _, y, _ in bands])
    eall = np.concatenate([np.asarray(e, dtype=float) for _, _, e in bands])
    ball = np.concatenate([np.full(len(t), k) for k, (t, _, _) in enumerate(bands)])
    perm = np.argsort(tout, kind="stable")
    for r in range(nb):
        om[r], b[r], V[r] = R._np_model(X[r], p, q)
        lag, a, mu = (np.asarray(v, dtype=float) for v in R._band_params(X[r], d, K))
        ao[r], muo[r] = a[band], mu[band]
        tcat = np.concatenate([tall - lag[ball], tout[perm] - lag[band]])
        scat = np.concatenate([ball, np.full(M, K)])
        o = np.lexsort((scat, tcat))                         # (stable: equal requested times keep their sorted order)
        dat = o < N
        tau[r] = tcat[o]
        src = np.where(dat, o, 0)
        yv[r] = np.where(dat, yall[src] - mu[ball[src]], 0.0)
        av[r] = np.where(dat, a[ball[src]], 1.0)
        ev[r] = np.where(dat, X[r, 1] * eall[src] ** 2, 1.0)
        slot[r] = np.where(dat, -1, perm[np.where(dat, 0, o - N)])
    isdat = slot < 0
    bc = np.conj(b)
    x = np.zeros((nb, p), dtype=complex)
    P = V.copy()
    U = np.empty((ng, nb, p), dtype=complex)
    RHO = np.ones((ng, nb, p), dtype=complex)
    S, VV, SX, F0 = (np.zeros((ng, nb)) for _ in range(4))
    for s in range(ng):
        if s:
            rho = np.exp(om * (tau[:, s] - tau[:, s - 1])[:, None])
            RHO[s] = rho
            x = rho * x
            P = rho[:, :, None] * np.conj(rho)[:, None, :] * (P - V) + V
        Pb = np.einsum("rij,rj->ri", P, bc)
        f = np.einsum("ri,ri->r", b, Pb).real
        sx = np.einsum("ri,ri->r", b, x).real
        var = av[:, s] ** 2 * f + ev[:, s]
        innov = yv[:, s] - av[:, s] * sx
        sv = np.where(isdat[:, s], 1.0 / var, 0.0)
        U[s], S[s], VV[s], SX[s], F0[s] = Pb, sv, innov, sx, f
        g = (av[:, s] * sv)[:, None] * Pb
        x = x + g * innov[:, None]
        P = P - (av[:, s] ** 2 * sv)[:, None, None] * Pb[:, :, None] * np.conj(Pb)[:, None, :]
    mean, var = np.empty((nb, M)), np.empty((nb, M))
    rr = np.zeros((nb, p), dtype=complex)
    NN = np.zeros((nb, p, p), dtype=complex)
    rows = np.arange(nb)
    for s in range(ng - 1, -1, -1):
        u = U[s]
        a_ = np.einsum("rij,rj->ri", NN, u)
        qn = np.einsum("ri,ri->r", np.conj(u), a_).real
        h = np.einsum("ri,ri->r", np.conj(u), rr).real
        rq = ~isdat[:, s]
        mean[rows[rq], slot[rq, s]] = (ao * (SX[s] + h) + muo)[rq]
        var[rows[rq], slot[rq, s]] = (ao * ao * (F0[s] - qn))[rq]
        g = av[:, s] ** 2 * S[s]                              # 0 at a requested time: r and N pass through
        rr = rr + bc * (av[:, s] * S[s] * (VV[s] - av[:, s] * h))[:, None]
        ga = g[:, None] * a_
        NN = (NN - ga[:, :, None] * b[:, None, :] - bc[:, :, None] * np.conj(ga)[:, None, :]
              + bc[:, :, None] * b[:, None, :] * (g + g * g * qn)[:, None, None])
        rho = RHO[s]
        rr = np.conj(rho) * rr
        NN = np.conj(rho)[:, :, None] * rho[:, None, :] * NN
    return (mean[0], var[0]) if np.ndim(thx) == 1 else (mean, var)


# ---- the requested times of the case table ---------------------------------------------------------------------------------------
M_TABLE = 12


def requested_times(bands, thx_row, p, q, band):
    """M = 12 observer times of band `band`, unsorted: two before all data and two behind (in shifted time), one exactly on the
    shifted time of a datum of ANOTHER band where there is one (a tie: exact where times and lags lie on the grid of 1/4), one
    in-between time twice, the rest in between."""
    K, d = len(bands), 3 + p + q
    lag, _, _ = R._band_params(thx_row, d, K)
    tau = np.concatenate([np.asarray(t, dtype=float) - lag[b] for b, (t, _, _) in enumerate(bands)])
    lo, hi = tau.min(), tau.max()
    other = (band + 1) % K
    j = len(bands[other][0]) // 2
    tie = float(bands[other][0][j]) - lag[other]
    between = [lo + f * (hi - lo) for f in (0.13, 0.31, 0.52, 0.64, 0.77, 0.9)]
    ts = [lo - 3.7, lo - 0.4, hi + 0.3, hi + 5.1, tie, between[1]] + between
    ts = np.array(ts) + lag[band]
    assert ts.size == M_TABLE
    return ts[np.random.default_rng(12).permutation(M_TABLE)]


def table_bands(K):
    """The output bands of a case: band 0 and the last band."""
    return sorted({0, K - 1})


@functools.lru_cache(None)
def smooth_case(p, q, name):
    """(bands, thx [2, dx], {band: (tout [12], mean [2, 12], var [2, 12])}) of a case: the exact values, computed once per process
    and shared by the tests that need them."""
    bands, thx, _ = R.case(p, q, name)
    out = {}
    for bo in table_bands(len(bands)):
        tout = requested_times(bands, thx[0], p, q, bo)      # (both rows of a case hold the same lags)
        mv = [dense_smooth_truth(bands, x, p, q, bo, tout) for x in thx]
        out[bo] = (tout, np.array([m for m, _ in mv]), np.array([v for _, v in mv]))
    return bands, thx, out


def errors(mean, var, tm, tv):
    """(largest mean error in units of max(|mean|, sd), largest relative variance error) against the exact tm, tv."""
    em = np.abs(np.asarray(mean) - tm) / np.maximum(np.abs(tm), np.sqrt(tv))
    ev = np.abs(np.asarray(var) - tv) / tv
    return float(np.max(em)), float(np.max(ev))
