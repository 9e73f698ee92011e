"""The estimators of carma_chain_diag restated in numpy, one column at a time: Goodman's `acor` autocorrelation time (MAXLAG 10,
WINMULT 5, MINFAC 5) with the status codes of the C entry point, and split R-hat (BDA3, no rank normalisation).  Test code only.

acor, level by level from the series itself (level 0): m = sum X / L, X <- X - m (at EVERY level); L < 50: status SHORT;
C[s] = sum_{i < L - 10} X[i] X[i + s] / (L - 10) for s = 0 ... 10; D = C[0] + 2 sum_{s >= 1} C[s], sigma = sqrt(D / L),
tau = D / C[0]; tau * 5 < 10: the last level; else X'[i] = X[2 i] + X[2 i + 1], i < L / 2, and again.  Unwinding, from the last
level back to level 0 with each enclosing level's own L and C[0]: D = 0.25 sigma^2 L, tau = D / C[0], sigma = sqrt(D / L).
Unlike the C original, which ignores the SHORT return of its recursive call, a SHORT level makes the column SHORT."""
import collections

import numpy as np

MAXLAG, WINMULT, MINFAC = 10, 5, 5
OK, SHORT, CONSTANT, NONFINITE = 0, 1, 2, 3

Acor = collections.namedtuple("Acor", "tau mean sigma status nlevels tau_last margin")


def acor(x):
    """One real series -> Acor(tau, mean, sigma, status, nlevels, tau_last, margin): nlevels = levels gone through, tau_last = tau_k
    of the last level, margin = the smallest |tau_k - 2| at any level (how far the nearest halving decision was from flipping)."""
    x = np.asarray(x, dtype=np.float64)
    L = x.size
    nan = float("nan")
    with np.errstate(all="ignore"):
        mean = float(np.sum(x) / L)
        if not np.all(np.isfinite(x)):
            return Acor(nan, mean, nan, NONFINITE, 0, nan, np.inf)
        X = x
        Ls, c0s = [], []
        margin, tau_k, D, nlev = np.inf, nan, nan, 0
        while True:
            Lk = X.size
            X = X - np.sum(X) / Lk
            nlev += 1
            if Lk < MINFAC * MAXLAG:
                return Acor(nan, mean, nan, SHORT, nlev, tau_k, margin)
            imax = Lk - MAXLAG
            C = np.array([np.sum(X[:imax] * X[s:s + imax]) / imax for s in range(MAXLAG + 1)])
            D = C[0] + 2.0 * np.sum(C[1:])
            if not Ls and C[0] == 0.0:
                return Acor(nan, mean, nan, CONSTANT, nlev, nan, margin)
            tau_k = D / C[0]
            Ls.append(Lk)
            c0s.append(C[0])
            margin = min(margin, abs(tau_k - 2.0)) if np.isfinite(tau_k) else margin
            if tau_k * WINMULT < MAXLAG:
                break
            h = Lk // 2
            X = X[0:2 * h:2] + X[1:2 * h:2]
        sigma = np.sqrt(D / Ls[-1])
        tau = tau_k
        for Lk, c0 in zip(Ls[-2::-1], c0s[-2::-1]):
            D = 0.25 * sigma * sigma * Lk
            tau = D / c0
            sigma = np.sqrt(D / Lk)
    return Acor(float(tau), mean, float(sigma), OK, nlev, float(tau_k), float(margin))


def split_rhat(chains):
    """chains [R, L] (one column of the R replicas of a group) -> split R-hat."""
    chains = np.asarray(chains, dtype=np.float64)
    R, L = chains.shape
    n = L // 2
    if n < 2 or not np.all(np.isfinite(chains)):
        return float("nan")
    halves = np.concatenate([chains[:, :n], chains[:, L - n:]], axis=0)
    W = np.mean(np.var(halves, axis=1, ddof=1))
    B = n * np.var(np.mean(halves, axis=1), ddof=1)
    if W == 0.0:
        return float("nan")
    return float(np.sqrt(((n - 1) / n * W + B / n) / W))


def chain_diag(x, rhat=True):
    """x [G, R, L, d] -> dict of tau, mean, sigma, status, nlevels, tau_last, margin [G, R, d] and rhat [G, d] (None without)."""
    x = np.asarray(x, dtype=np.float64)
    G, R, L, d = x.shape
    out = {k: np.empty((G, R, d), dtype=np.int32 if k in ("status", "nlevels") else np.float64) for k in Acor._fields}
    for g in range(G):
        for r in range(R):
            for c in range(d):
                a = acor(x[g, r, :, c])
                for k in Acor._fields:
                    out[k][g, r, c] = getattr(a, k)
    out["rhat"] = np.array([[split_rhat(x[g, :, :, c]) for c in range(d)] for g in range(G)]) if rhat else None
    return out


def ar1(rng, L, phi, offset=0.0):
    """x[i] = phi x[i - 1] + e[i] with unit normal e, started from the stationary distribution, plus `offset`.  phi and offset
    may be arrays [...]: then x is [L, ...], every trailing index its own chain."""
    phi, offset = np.asarray(phi, dtype=np.float64), np.asarray(offset, dtype=np.float64)
    e = rng.standard_normal((L,) + phi.shape)
    x = np.empty_like(e)
    x[0] = e[0] / np.sqrt(1.0 - phi * phi)
    for i in range(1, L):
        x[i] = phi * x[i - 1] + e[i]
    return x + offset


def ar1_block(seed, G, R, L, phis, offsets):
    """[G, R, L, d] with column c an AR(1) of phis[c] plus offsets[c], every chain its own draw from default_rng(seed)."""
    d = len(phis)
    x = ar1(np.random.default_rng(seed), L, np.broadcast_to(np.asarray(phis, dtype=float), (G, R, d)),
            np.broadcast_to(np.asarray(offsets, dtype=float), (G, R, d)))
    return np.ascontiguousarray(np.moveaxis(x, 0, 2))
