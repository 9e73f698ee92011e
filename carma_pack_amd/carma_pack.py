"""carma_pack's Python API (src/carmcmc/carma_pack.py in the reference) on top of the MI355X path.

Same public names and call signatures -- ``CarmaModel`` (``run_mcmc``, ``get_mle``, ``choose_order``),
``CarmaSample`` / ``Car1Sample`` (``get_samples``, ``parameters``, ``mle``, derived quantities),
``get_ar_roots``, ``power_spectrum``, ``carma_variance``, ``car1_process``, ``carma_process`` -- but a
fresh implementation: derived quantities are vectorised numpy, every log-density goes through one
batched launch, the sampler runs on the GPU, and ``run_mcmc``/``get_mle`` can use many independent
replicas at once (``nreplicas``).  ``predict``/``simulate``/``assess_fit`` use the batched device
Predict kernel (one launch for all requested times); plotting bodies are not part of the hot path.
"""
import os
from time import perf_counter

import numpy as np
from scipy.optimize import minimize

from . import _carmcmc as carmcmcLib
from ._lib import _bounds_lohi, _times_per_row, _which

__all__ = ["CarmaModel", "CarmaModelSet", "CarmaBandsModel", "CarmaBandsSample", "CarmaBandsSet", "CarmaSample", "Car1Sample", "MCMCSample", "get_ar_roots", "power_spectrum",
           "carma_variance", "car1_process", "carma_process", "carma_process_batch", "car1_process_batch", "mle_to_model"]


# ------------------------------------------------------------------------------------------------
# free functions (reference: carma_pack.py:1038-1259)
def get_ar_roots(qpo_width, qpo_centroid):
    """Lorentzian widths/centroids -> roots of the AR polynomial, -2 pi (width + i centroid) with the
    conjugate appended for every centroid > 1e-10 and one extra real root when there is one more width
    than centroids (reference :1038-1059)."""
    qpo_width, qpo_centroid = np.atleast_1d(qpo_width), np.atleast_1d(qpo_centroid)
    roots = []
    for w, c in zip(qpo_width, qpo_centroid):
        roots.append(w + 1j * c)
        if c > 1e-10:
            roots.append(w - 1j * c)
    if qpo_width.size - qpo_centroid.size == 1:
        roots.append(qpo_width[-1] + 0j)
    return -2.0 * np.pi * np.array(roots)


def power_spectrum(freq, sigma, ar_coef, ma_coefs=(1.0,)):
    """sigma^2 |beta(2 pi i f)|^2 / |alpha(2 pi i f)|^2 (reference :1062-1081); ar_coef highest order
    first (np.poly convention), ma_coefs lowest order first."""
    s = 2.0j * np.pi * np.asarray(freq, dtype=float)
    num = np.polyval(np.asarray(ma_coefs)[::-1], s)
    den = np.polyval(np.asarray(ar_coef), s)
    return sigma ** 2 * np.abs(num) ** 2 / np.abs(den) ** 2


def carma_variance(sigsqr, ar_roots, ma_coefs=(1.0,), lag=0.0):
    """Autocovariance of a CARMA(p,q) process at `lag` (reference :1084-1123 == CARp::Variance,
    src/carpack.cpp:377-409)."""
    r = np.asarray(ar_roots, dtype=complex)
    p = r.size
    beta = np.zeros(p)
    beta[:len(ma_coefs)] = ma_coefs
    powers = np.arange(p)
    total = 0.0 + 0.0j
    for k in range(p):
        others = np.delete(r, k)
        denom = -2.0 * r[k].real * np.prod((others - r[k]) * (np.conj(others) + r[k]))
        num = np.sum(beta * r[k] ** powers) * np.sum(beta * (-r[k]) ** powers) * np.exp(r[k] * abs(lag))
        total += num / denom
    return sigsqr * total.real


def car1_process(time, sigsqr, tau, rng=None):
    """Exact Ornstein-Uhlenbeck draw at the given times (reference :1126-1146)."""
    rng = np.random if rng is None else rng
    time = np.asarray(time, dtype=float)
    var = sigsqr * tau / 2.0
    y = np.empty(time.size)
    y[0] = np.sqrt(var) * rng.standard_normal()
    rho = np.exp(-np.diff(time) / tau)
    eps = rng.standard_normal(time.size - 1)
    for i in range(1, time.size):
        y[i] = rho[i - 1] * y[i - 1] + np.sqrt(var * (1.0 - rho[i - 1] ** 2)) * eps[i - 1]
    return y


def _rotated_system(sigsqr, ar_roots, ma_coefs):
    """Diagonalised state space of kfilter.cpp:138-172: returns (b, V) with V Hermitian."""
    r = np.asarray(ar_roots, dtype=complex)
    p = r.size
    E = np.vander(r, p, increasing=True).T           # E[i, j] = r_j ** i
    e = np.zeros(p, dtype=complex)
    e[-1] = 1.0
    J = np.linalg.solve(E, e)
    beta = np.zeros(p)
    beta[:len(ma_coefs)] = ma_coefs
    b = beta @ E
    V = -sigsqr * np.outer(J, np.conj(J)) / (r[:, None] + np.conj(r)[None, :])
    return b, V


def carma_process(time, sigsqr, ar_roots, ma_coefs=(1.0,), rng=None):
    """Draw a CARMA(p,q) path at the (sorted) times by sequential conditional simulation: each value
    is drawn from its one-step predictive distribution (same construction as reference :1148-1259,
    written with the D = P - V recursion used by the device kernel)."""
    rng = np.random if rng is None else rng
    r = np.asarray(ar_roots, dtype=complex)
    time = np.sort(np.asarray(time, dtype=float))
    if r.size == 1:
        return car1_process(time, sigsqr, -1.0 / r.real.item(), rng)
    b, V = _rotated_system(sigsqr, r, ma_coefs)
    c = V @ np.conj(b)
    s0 = float(np.real(b @ c))
    p = r.size
    D = np.zeros((p, p), dtype=complex)
    x = np.zeros(p, dtype=complex)
    y = np.empty(time.size)
    var, mean = s0, 0.0
    y[0] = rng.normal(mean, np.sqrt(var))
    innov = y[0] - mean
    u = c.copy()
    for k in range(1, time.size):
        rho = np.exp(r * (time[k] - time[k - 1]))
        if var > 0.0:
            x = rho * (x + u * (innov / var))
            D = np.outer(rho, np.conj(rho)) * (D - np.outer(u, np.conj(u)) / var)
        else:                                        # the previous value was known: no measurement update
            x = rho * x
            D = np.outer(rho, np.conj(rho)) * D
        w = D @ np.conj(b)
        u = w + c
        # a repeated time has one-step variance exactly 0 (the value repeats); in doubles it comes out at rounding size,
        # of either sign (the reference's np.sqrt then yields NaN) -- same rule as the device (carma_simulate.h)
        var = 0.0 if time[k] == time[k - 1] else s0 + float(np.real(b @ w))
        mean = float(np.real(b @ x))
        y[k] = rng.normal(mean, np.sqrt(max(var, 0.0)))
        innov = y[k] - mean
    return y


def carma_process_batch(time, sigsqr, ar_roots, ma_coefs=(1.0,), npaths=1, seed=0, device=None):
    """`npaths` independent draws of carma_process in ONE launch on the GPU (carma_simulate_carma: the same
    value-by-value construction, reference :1148-1259, normal variates from the counter-based generator keyed by
    (seed, path, step)).  Returns [npaths][n] at the sorted times."""
    from . import _lib
    r = np.atleast_1d(np.asarray(ar_roots, dtype=complex))
    if r.size == 1:
        return car1_process_batch(time, sigsqr, -1.0 / r.real.item(), npaths, seed, device)
    return _lib.simulate_carma(time, sigsqr, r, np.asarray(ma_coefs, dtype=float), npaths, seed, device)


def car1_process_batch(time, sigsqr, tau, npaths=1, seed=0, device=None):
    """`npaths` independent Ornstein-Uhlenbeck paths (car1_process, reference :1126-1146) in one launch."""
    from . import _lib
    return _lib.simulate_car1(time, sigsqr, 1.0 / tau, npaths, seed, device)


# ------------------------------------------------------------------------------------------------
class BatchResult(object):
    """scipy.optimize.OptimizeResult look-alike for one start of the lock-step optimiser (carma_mle_batched)."""

    def __init__(self, x, fun, nit, nfev, success, message):
        self.x, self.fun, self.nit, self.nfev, self.success, self.message = x, fun, nit, nfev, success, message

    def __repr__(self):
        return "BatchResult(fun=%r, nit=%d, success=%r)" % (self.fun, self.nit, self.success)


# status codes of carma_mle_batched (include/carma_mi355.h) in words
STATUS_TEXT = ("converged: projected gradient <= gtol", "converged: relative reduction of f <= ftol",
               "maximum number of iterations reached", "line search failed", "no finite value at the start")


# ---- what the model classes share: no object state, so plain functions -----------------------------------
def mle_bounds(time, y, p, q):
    """L-BFGS-B box of the reference (:219-240) for a CARMA(p,q) fit of the series (time sorted, at least two distinct)."""
    ysigma = y.std()
    dt = np.diff(time)
    max_freq, min_freq = 0.9 / dt.min(), 1.0 / (time.max() - time.min())
    bnds = [(ysigma / 10.0, 10.0 * ysigma), (0.9, 1.1), (None, None)]
    if p == 1:
        bnds.append((np.log(min_freq), np.log(max_freq)))
    else:
        lo = np.log(min(min_freq ** 2, 2.0 * min_freq))
        hi = np.log(max(max_freq ** 2, 2.0 * max_freq))
        bnds += [(lo, hi)] * p + [(None, None)] * q
    return bnds


def _clamp_starts(starts, bnds, seed):
    """A short sampler run's draws [ntrials, d] -> the starts of get_mle, in place (reference :195-240): the error scale set to
    1 (:217), an entry outside its box `bnds` drawn anew, uniform in the box, from np.random.default_rng(seed)."""
    rng = np.random.default_rng(seed)
    starts[:, 1] = 1.0
    for j, (lo, hi) in enumerate(bnds):
        if lo is not None:
            out = (starts[:, j] < lo) | (starts[:, j] > hi)
            starts[out, j] = rng.uniform(lo, hi, int(out.sum()))
    return starts


def _batch_results(xs, fs, nits, nfevs, sts):
    """What a context's mle_batched returns -> one BatchResult per start."""
    return [BatchResult(xs[i].copy(), float(fs[i]), int(nits[i]), int(nfevs[i]), int(sts[i]) < 2, STATUS_TEXT[int(sts[i])])
            for i in range(xs.shape[0])]


def _best_result(results):
    """The best finite result, else the best."""
    return min([r for r in results if np.isfinite(r.fun) and r.fun < 1e299] or results, key=lambda r: r.fun)


def _results_per_member(res, S, nt, return_all):
    """mle_batched's answer for S members of a set with nt starts each, back to back -> S best results (return_all: S lists)."""
    results = _batch_results(*res)
    groups = [results[s * nt:(s + 1) * nt] for s in range(S)]
    return groups if return_all else [_best_result(g) for g in groups]


def _pq_grid(pmax, qmax, pqlist):
    """The orders choose_order tries (reference :131-192): pqlist, or every (p, q) with p <= pmax, q < p, q <= qmax."""
    if pmax < 1:
        raise ValueError("Order of AR polynomial must be at least 1.")
    if qmax is None:
        qmax = pmax - 1
    if pqlist is None:
        pqlist = [(p, q) for p in range(1, pmax + 1) for q in range(min(p, qmax + 1))]
    return pqlist


def aicc(fun, p, q, n):
    """AICc of a CARMA(p,q) fit with objective value fun = -loglik to n data (reference :131-192)."""
    k = 2 + p + q
    return 2.0 * k + 2.0 * fun + 2.0 * k * (k + 1.0) / (n - k - 1.0)


def _choose_order(mles, pqlist, n):
    """(best fit, AICc of every order, the order of the best -- None when no AICc is below 1e300) of one series of n data."""
    AICc = [aicc(mle.fun, p, q, n) for mle, (p, q) in zip(mles, pqlist)]
    best, order, best_aicc = mles[0], None, 1e300
    for mle, pq, a in zip(mles, pqlist, AICc):
        if a < best_aicc:
            best, order, best_aicc = mle, pq, a
    return best, AICc, order


def _series_item(item, noun, k, least=0):
    """One (time, y, ysig) of a constructor's list -> three flat float arrays of one length (`least`: at least that many)."""
    if len(item) != 3:
        raise ValueError("%s %d: expected (time, y, ysig)" % (noun, k))
    t, y, e = (np.asarray(a, dtype=float).ravel() for a in item)
    if not (t.size == y.size == e.size) or t.size < least:
        raise ValueError("%s %d: time, y, ysig must have the same length%s" % (noun, k, ", at least %d" % least if least else ""))
    return t, y, e


def _resolve_samples(samples, kept, S):
    """samples= of the set's post-processing calls: the caller's list of S sample objects, by default what run_mcmc kept."""
    if samples is None:
        samples = kept
        if samples is None:
            raise ValueError("no samples: call run_mcmc first, or pass samples=")
    samples = list(samples)
    if len(samples) != S:
        raise ValueError("samples must hold one sample object per series (%d), got %d" % (S, len(samples)))
    return samples


def _lag_grid(lags, K, lag_bounds, obj=None):
    """lags of lag_profile ([L] for two bands, else [L, K - 1]) -> [L, K - 1], every lag inside its box.  obj: the object of a
    set the grid is for, as the messages name it."""
    g = np.asarray(lags, dtype=float)
    g = g.reshape(-1, 1) if K == 2 and g.ndim == 1 else np.atleast_2d(g)
    if g.shape[1] != K - 1:
        raise ValueError("lags must be [L] for two bands or [L, %d]%s"
                         % (K - 1, "" if obj is None else ", for all objects or a list of one per object"))
    if not np.all((g >= lag_bounds[:, 0]) & (g <= lag_bounds[:, 1])):
        raise ValueError("%severy lag must lie inside its box (lag_bounds)" % ("" if obj is None else "object %d: " % obj))
    return g


def _profile_best(fs, xs, L, nt):
    """The objective values fs [L x nt] and optima xs of a lag profile, nt starts per lag -> (loglik [L], x [L, dx]): the best
    start of every lag; a start without a finite value never wins."""
    fs = np.where(np.isfinite(fs), fs, 1e300).reshape(L, nt)
    best = fs.argmin(axis=1)
    return -fs[np.arange(L), best], xs.reshape(L, nt, xs.shape[1])[np.arange(L), best]


def _timing(t0, t1, t2):
    """perf_counter() before the starts, after them and after the optimiser -> what get_mle / lag_profile keep as self.timing."""
    return {"starts_s": t1 - t0, "optimise_s": t2 - t1}


def _mcmc_defaults(nsamples, nburnin, ntemperatures, p, q):
    """(nburnin, ntemperatures) with run_mcmc's defaults as the reference has them (:53-89): nsamples / 2 and max(10, p + q)."""
    return nsamples // 2 if nburnin is None else nburnin, max(10, p + q) if ntemperatures is None else ntemperatures


def _mcmc_args(nsamples, nburnin, ntemperatures, nthin, nreplicas, p, q):
    """The sampler arguments of a run_mcmc on a lane sampler, defaults filled in, as ints, refused here before any library call
    -> (nsamples, nburnin, ntemperatures, nthin, nreplicas)."""
    nsamples, nthin, nreplicas = int(nsamples), int(nthin), int(nreplicas)
    if nsamples < 1:
        raise ValueError("nsamples must be at least 1")
    if nthin < 1:
        raise ValueError("nthin must be at least 1")
    if nreplicas < 1:
        raise ValueError("nreplicas must be at least 1")
    nburnin, ntemperatures = (int(v) for v in _mcmc_defaults(nsamples, nburnin, ntemperatures, p, q))
    if not 1 <= ntemperatures <= 64:
        raise ValueError("ntemperatures must be 1 ... 64 (a ladder is the lanes of one wave), got %d" % ntemperatures)
    if nburnin < 0:
        raise ValueError("nburnin must not be negative")
    return nsamples, nburnin, ntemperatures, nthin, nreplicas


def _band_bounds(name, v, K, positive=False):
    """run_mcmc's scale_bounds ((lo, hi) of a_b, `positive`) or offset_bounds ((lo, hi) of mu_b) -- `name` for the messages --
    one pair per band after the first, checked -> [K - 1, 2]; None stays None (the default box)."""
    if v is None:
        return None
    a = np.asarray(v, dtype=float)
    if a.shape != (K - 1, 2):
        raise ValueError("%s must hold one (lo, hi) pair for each of the %d bands after the first, got shape %r" % (name, K - 1, a.shape))
    if not np.all(a[:, 0] <= a[:, 1]) or (positive and not np.all(a[:, 0] > 0)):
        raise ValueError("%s: need %slo <= hi in every pair" % (name, "0 < " if positive else ""))
    return a


def _sampler_box(default, scale_bounds, offset_bounds):
    """A context's default box (lo, hi) [K - 1, 2], columns (log a_b, mu_b), with the checked scale_bounds / offset_bounds of
    run_mcmc put in where given -> the (lo, hi) the context's sampler takes."""
    lo, hi = default
    if scale_bounds is not None:
        lo[:, 0], hi[:, 0] = np.log(scale_bounds[:, 0]), np.log(scale_bounds[:, 1])
    if offset_bounds is not None:
        lo[:, 1], hi[:, 1] = offset_bounds[:, 0], offset_bounds[:, 1]
    return lo, hi


class MCMCSample(object):
    """Minimal sample container (the reference's samplers.MCMCSample holds the same `_samples` dict; its plotting methods are
    outside the hot path, its two diagnostics -- autocorr_timescale, effective_samples -- run on the device)."""

    def __init__(self, filename=None, logpost=None, trace=None):
        # reference samplers.py:27-45: a trace wins over a file name
        self._samples = {}
        if trace is not None:
            self.generate_from_trace(trace)
        elif filename is not None:
            self.generate_from_file([filename])
        if logpost is not None:
            self.set_logpost(logpost)

    def get_samples(self, name):
        return self._samples[name].copy()

    def generate_from_file(self, filename):
        """One parameter per ascii file, its name on the first line (reference samplers.py:57-72).  `filename` is a
        list of file names."""
        for fname in filename:
            with open(fname, "r") as f:
                name = f.readline()
            trace = np.genfromtxt(fname, skip_header=1)
            if name not in self._samples:
                self._samples[name] = trace

    def set_logpost(self, logpost):
        self._samples["logpost"] = np.asarray(logpost)

    def newaxis(self):
        for k, v in self._samples.items():
            if v.ndim == 1:
                self._samples[k] = v[:, np.newaxis]

    def posterior_summaries(self, name):
        s = self._samples[name]
        out = dict(median=np.median(s, axis=0), mean=np.mean(s, axis=0), std=np.std(s, axis=0),
                   ci68=np.percentile(s, [16.0, 84.0], axis=0), ci95=np.percentile(s, [2.5, 97.5], axis=0))
        return out


    def autocorr_timescale(self, trace):
        """The autocorrelation time of every column of a trace ([ns] or [ns, k]; the real part of a complex one), as estimated
        by Goodman's `acor` (reference samplers.py:74-84) -- all columns in one device call (carma_chain_diag).  A column the
        estimator has no answer for (too short, constant, non-finite: chain_diag's status) comes back NaN."""
        trace = np.asarray(trace)
        if trace.ndim not in (1, 2):
            raise ValueError("trace must be [ns] or [ns, k], got %d axes" % trace.ndim)
        if trace.ndim == 1:
            trace = trace[:, None]
        return carmcmcLib.chain_diag(np.ascontiguousarray(trace.real, dtype=float), rhat=False)["tau"][0, 0]

    def effective_samples(self, name):
        """The effective number of independent samples of parameter `name`: ns / autocorr_timescale, per column (reference
        samplers.py:86-101).  An unknown name is a KeyError."""
        if name not in self._samples:
            raise KeyError("sampler does not have %r" % (name,))
        traces = self._samples[name]
        return traces.shape[0] / self.autocorr_timescale(traces)


def _diagnostics_of(par, lp):
    """chain_diag results of the parameter columns (par) and of the log-posterior column (lp) joined: the columns are the
    parameter vector followed by logpost."""
    return {k: np.concatenate([par[k], lp[k]], axis=-1) for k in ("tau", "mean", "sigma", "status", "rhat")}


def _ess_of(tau, status, L):
    """Sum over the replicas (the last axis but one) of L / tau; NaN where a replica's status is not 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ess = np.sum(L / tau, axis=-2)
    ess[np.any(status != 0, axis=-2)] = np.nan
    return ess


def _roots_from_log_quads(logq):
    """[nsamples, m] log quadratic-factor coefficients -> [nsamples, m] complex roots
    (CARp::ARRoots ordering, src/carpack.cpp:137-172)."""
    logq = np.atleast_2d(logq)
    ns, m = logq.shape
    quad = np.exp(logq)
    roots = np.empty((ns, m), dtype=complex)
    for i in range(m // 2):
        q1, q2 = quad[:, 2 * i], quad[:, 2 * i + 1]
        disc = q2 * q2 - 4.0 * q1
        sq = np.where(disc > 0, np.sqrt(np.abs(disc)) + 0j, 1j * np.sqrt(np.abs(disc)))
        roots[:, 2 * i] = -0.5 * (q2 + sq)
        # two real roots: the smaller one from the product q1 (as the kernels do, carma_core.h quad_root) --
        # -(q2 - sq) / 2 cancels to nothing once q2^2 >> 4 q1
        with np.errstate(divide="ignore", invalid="ignore"):
            roots[:, 2 * i + 1] = np.where((disc > 0) & (q2 - sq != 0), q1 / roots[:, 2 * i], -0.5 * (q2 - sq))
    if m % 2:
        roots[:, -1] = -quad[:, -1]
    return roots


def _poly_from_roots(roots):
    """Vectorised np.poly over the first axis: [ns, m] roots -> [ns, m+1] coefficients, highest first."""
    ns, m = roots.shape
    coefs = np.zeros((ns, m + 1), dtype=complex)
    coefs[:, 0] = 1.0
    for i in range(m):
        coefs[:, 1:i + 2] = coefs[:, 1:i + 2] - roots[:, i:i + 1] * coefs[:, 0:i + 1]
    return coefs


def mle_to_model(x, p, q=0):
    """An MLE parameter vector x of order (p, q) -> (sigsqr, ar_roots, ma_coefs, mu): the model of the Kalman filter, derived
    exactly as CarmaSample.add_mle derives it -- var = x[0]^2, roots and MA coefficients from the log quadratic factors,
    sigsqr = var / carma_variance(1, roots, ma); CAR(1): omega = exp(x[3]), sigsqr = 2 omega var, the one root -omega."""
    x = np.asarray(x, dtype=float).ravel()
    p, q = int(p), int(q)
    d = 4 if p == 1 else 3 + p + q
    if p < 1 or q < 0 or q >= p or x.size != d:
        raise ValueError("mle_to_model: a CARMA(%d,%d) parameter vector has %d entries, got %d" % (p, q, d, x.size))
    var, mu = x[0] ** 2, float(x[2])
    if p == 1:
        omega = np.exp(x[3])
        return float(2.0 * omega * var), np.array([-omega + 0j]), np.ones(1), mu
    roots = _roots_from_log_quads(x[None, 3:p + 3])[0]
    if q == 0:
        ma = np.ones(1)
    else:
        c = np.poly(_roots_from_log_quads(x[None, 3 + p:])[0])
        ma = np.real(c / c[q])[::-1]
    return float(var / carma_variance(1.0, roots, ma)), roots, ma, mu


def group_by_order(orders):
    """[(p, q)] per series -> {(p, q): [series indices]}, orders in order of first appearance."""
    groups = {}
    for s, (p, q) in enumerate(orders):
        groups.setdefault((int(p), int(q)), []).append(s)
    return groups


class CarmaSample(MCMCSample):
    """MCMC samples of a CARMA(p,q) model plus derived quantities (reference :263-546)."""

    def __init__(self, time, y, ysig, sampler, q=0, filename=None, MLE=None):
        self.time, self.y, self.ysig, self.q = time, y, ysig, q
        self._sampler = sampler
        logpost = np.array(sampler.GetLogLikes())
        trace = np.array(sampler.getSamples())
        # (as in the reference, :290, `filename` only matters when the sampler holds no trace: generate_from_file below
        # reads the ascii file the C++ carpack wrote)
        super(CarmaSample, self).__init__(filename=filename, logpost=logpost, trace=trace)
        self._ar_roots()
        self._ar_coefs()
        self._ma_coefs(trace)
        self._sigma_noise()
        # "loglik": LogDensity with the prior bounds ignored -- still includes the measurement-error
        # prior, exactly as the reference computes it (:305-315, carpack.hpp:173).  One batched launch.
        if hasattr(sampler, "SetMLE"):
            sampler.SetMLE(True)
        self._samples["loglik"] = np.asarray(sampler.getLogDensityBatch(trace))
        self.parameters = list(self._samples.keys())
        self.newaxis()
        self.mle = {}
        if MLE is not None:
            self.add_mle(MLE)

    def generate_from_file(self, filename):
        """Samples from an ascii file written by the C++ carpack: one header line, then one row per sample holding the
        parameter vector followed by the log-posterior (reference :427-437; `filename` is a list, its first entry is
        read)."""
        trace = np.atleast_2d(np.genfromtxt(filename[0], skip_header=1))
        self.generate_from_trace(trace[:, 0:-1])
        self.set_logpost(trace[:, -1])

    def generate_from_trace(self, trace):
        self.p = trace.shape[1] - 3 - self.q          # sic: p inferred from the trace width (:415)
        self._samples["var"] = trace[:, 0] ** 2
        self._samples["measerr_scale"] = trace[:, 1]
        self._samples["mu"] = trace[:, 2]
        self._samples["quad_coefs"] = np.exp(trace[:, 3:self.p + 3])

    def _ar_roots(self):
        roots = _roots_from_log_quads(np.log(self._samples["quad_coefs"]))
        self._samples["ar_roots"] = roots
        self._samples["psd_centroid"] = np.abs(roots.imag) / (2.0 * np.pi)
        self._samples["psd_width"] = -roots.real / (2.0 * np.pi)

    def _ar_coefs(self):
        self._samples["ar_coefs"] = _poly_from_roots(self._samples["ar_roots"]).real

    @staticmethod
    def _ma_coefs_of(trace, p, q):
        """[ns, q + 1] MA coefficients, lowest order first and scaled to a leading 1, of the rows of a trace."""
        if q == 0:
            return np.ones((trace.shape[0], 1))
        roots = _roots_from_log_quads(trace[:, 3 + p:3 + p + q])
        c = _poly_from_roots(roots)
        return (c / c[:, q:q + 1])[:, ::-1].real

    def _ma_coefs(self, trace):
        self._samples["ma_coefs"] = self._ma_coefs_of(trace, self.p, self.q)

    @staticmethod
    def _sigma_inputs_of(trace, p, q):
        """(ar_roots, ma_coefs, var) of the rows of a trace, derived step by step as the constructor derives the entries of
        `_samples` that _sigma_noise reads."""
        quad = np.exp(trace[:, 3:p + 3])
        return _roots_from_log_quads(np.log(quad)), CarmaSample._ma_coefs_of(trace, p, q), trace[:, 0] ** 2

    def _sigma_noise(self):
        """sigma of the driving noise per sample = sqrt(var / Variance(roots, ma, 1)) (reference :513-546): one launch for all
        samples (carma_sigma_noise_batch) -- unless the sampler holds them already, computed with those of the other series of
        a set in one launch (SetRunSampler.getSigmaNoise)."""
        args = self._samples["ar_roots"], self._samples["ma_coefs"], self._samples["var"]
        offer = getattr(self._sampler, "getSigmaNoise", None)
        sigma = offer(*args) if offer is not None else None
        self._samples["sigma"] = carmcmcLib.sigma_noise_batch(*args) if sigma is None else sigma

    def diagnostics(self):
        """Has the run mixed?  Over ALL replicas of the run (getAllSamples of the wrapped sampler), per column of the sampler's
        own parameter vector followed by logpost as the last column: tau [R, d + 1] (acor autocorrelation time), ess [d + 1]
        (sum over the replicas of L / tau; NaN where a replica's status is not 0), rhat [d + 1] (split R-hat over the
        replicas), status [R, d + 1], mean and sigma [R, d + 1] -- two device calls (carma_chain_diag)."""
        samples, logposts = self._sampler.getAllSamples()
        if samples is None:
            raise ValueError("the sampler holds no samples")
        samples, logposts = np.asarray(samples, dtype=float), np.asarray(logposts, dtype=float)
        out = _diagnostics_of(carmcmcLib.chain_diag(samples[None]), carmcmcLib.chain_diag(logposts[None, :, :, None]))
        out = {k: v[0] for k, v in out.items()}
        out["ess"] = _ess_of(out["tau"], out["status"], samples.shape[1])
        return out

    def add_mle(self, MLE):
        x = np.asarray(MLE.x, dtype=float)
        roots = _roots_from_log_quads(x[None, 3:self.p + 3])[0]
        self.mle = {"loglik": -MLE.fun, "var": x[0] ** 2, "measerr_scale": x[1], "mu": x[2], "ar_roots": roots,
                    "psd_width": -roots.real / (2 * np.pi), "psd_cent": np.abs(roots.imag) / (2 * np.pi),
                    "ar_coefs": np.poly(roots).real}
        if self.q == 0:
            self.mle["ma_coefs"] = 1.0
        else:
            mr = _roots_from_log_quads(x[None, 3 + self.p:])[0]
            c = np.poly(mr)
            self.mle["ma_coefs"] = np.real(c / c[self.q])[::-1]
        unit = carma_variance(1.0, roots, np.atleast_1d(self.mle["ma_coefs"]))
        self.mle["sigma"] = np.sqrt(self.mle["var"] / unit)

    def DIC(self):
        """Deviance information criterion from the stored log-likelihoods."""
        loglik = self._samples["loglik"].ravel()
        dev = -2.0 * loglik
        return float(np.mean(dev) + 0.5 * np.var(dev))

    def _psd_frequencies(self, nfreq=1000):
        """Log-spaced grid between 1 / (time span) and 0.5 / (smallest time step) (reference :583-594)."""
        dt_min = np.diff(self.time).min()
        dt_max = self.time.max() - self.time.min()
        return np.exp(np.linspace(np.log(1.0 / dt_max), np.log(0.5 / dt_min), num=nfreq))

    @staticmethod
    def _subsample(nsamples, nsamples0):
        """The evenly spaced sample indices the reference uses when nsamples < all (:572-578)."""
        if nsamples is None or nsamples >= nsamples0:
            return np.arange(nsamples0)
        return (np.arange(nsamples) * (nsamples0 / nsamples)).astype(int)

    def _psd_inputs(self, index):
        sig = np.ravel(self._samples["sigma"])[index]
        return self._samples["ar_coefs"][index], self._samples["ma_coefs"][index], sig

    def _psd_samples(self, frequencies, index):
        """sigma^2 |delta(2 pi i f)|^2 / |alpha(2 pi i f)|^2 for every (frequency, sample) pair (reference :601-618): the
        [nfreq, nsamples] grid from the device (carma_psd_band without percentiles)."""
        ar, ma, sig = self._psd_inputs(index)
        return carmcmcLib.psd_band(ar, ma, sig, frequencies, [], return_samples=True)[1]

    def _psd_credint(self, percentile, nsamples, frequencies):
        """(lower, median, upper) of the spectrum over the samples at every frequency (reference :596-623): grid and
        percentiles on the device, one call (carma_psd_band)."""
        index = self._subsample(nsamples, self._samples["sigma"].shape[0])
        lower = (100.0 - percentile) / 2.0
        ar, ma, sig = self._psd_inputs(index)
        return carmcmcLib.psd_band(ar, ma, sig, frequencies, [lower, 50.0, 100.0 - lower])

    def plot_power_spectrum(self, percentile=68.0, nsamples=None, plot_log=True, color="b", alpha=0.5, sp=None,
                            doShow=True):
        """Posterior median and `percentile` credibility band of the power spectrum on 1000 log-spaced frequencies
        (reference :548-648).  Returns the reference's tuple (lower PSD, upper PSD, median PSD, frequencies).  The
        numbers are computed for every (frequency, sample) pair at once; drawing happens only when a subplot is
        passed or doShow is true (matplotlib is imported lazily -- plotting is not part of the hot path)."""
        frequencies = self._psd_frequencies()
        ci = self._psd_credint(percentile, nsamples, frequencies)
        if sp is not None or doShow:
            import matplotlib.pyplot as plt
            if sp is None:
                sp = plt.figure().add_subplot(111)
            (sp.loglog if plot_log else sp.plot)(frequencies, ci[:, 1], color=color)
            sp.fill_between(frequencies, ci[:, 2], ci[:, 0], facecolor=color, alpha=alpha)
            sp.set_xlim(frequencies.min(), frequencies.max())
            sp.set_xlabel("Frequency")
            sp.set_ylabel("Power Spectrum")
            if doShow:
                plt.show()
        return ci[:, 0], ci[:, 2], ci[:, 1], frequencies

    def power_spectrum_band(self, percentile=68.0, nsamples=None, freq=None):
        """plot_power_spectrum's numbers on a caller-chosen frequency grid, without any drawing."""
        frequencies = self._psd_frequencies() if freq is None else np.asarray(freq, dtype=float)
        ci = self._psd_credint(percentile, nsamples, frequencies)
        return ci[:, 0], ci[:, 2], ci[:, 1], frequencies

    def _point_params(self, bestfit):
        """(sigsqr, mu, ar_roots, ma_coefs) of a point estimate: 'map', 'median', 'mean', a sample index, or -- any other
        string, 'random' by convention -- one sample drawn from numpy's global stream (reference :650-676)."""
        if bestfit == "map":
            i = int(np.argmax(self._samples["logpost"]))
            pick = lambda a: a[i]  # noqa: E731
        elif bestfit == "median":
            pick = lambda a: np.median(a, axis=0)  # noqa: E731
        elif bestfit == "mean":
            pick = lambda a: np.mean(a, axis=0)  # noqa: E731
        elif isinstance(bestfit, str):
            i = int(np.random.randint(0, self._samples["sigma"].shape[0]))    # a random draw from the posterior (:670-676)
            pick = lambda a: a[i]  # noqa: E731
        else:
            pick = lambda a: a[int(bestfit)]  # noqa: E731
        sigsqr = float(np.ravel(pick(self._samples["sigma"]))[0]) ** 2
        mu = float(np.ravel(pick(self._samples["mu"]))[0])
        roots = np.atleast_1d(pick(self._samples["ar_roots"]))
        ma = np.atleast_1d(pick(self._samples["ma_coefs"]))
        return sigsqr, mu, roots, ma

    def makeKalmanFilter(self, bestfit):
        """KalmanFilterp for a point estimate ('map', 'median', 'mean' or a sample index) or, for any other string
        ('random'), for one random draw from the posterior; reference :650-685."""
        sigsqr, mu, roots, ma = self._point_params(bestfit)
        omega = carmcmcLib.vecC(roots.tolist())
        kf = carmcmcLib.KalmanFilterp(carmcmcLib.vecD(self.time), carmcmcLib.vecD(self.y - mu),
                                      carmcmcLib.vecD(self.ysig), sigsqr, omega, carmcmcLib.vecD(ma.tolist()))
        return kf, mu

    def _path_models(self, index):
        """Model arrays of the samples `index` as the conditional simulation takes them: (sigsqr, mu, (ar_roots, ma_coefs))."""
        sig = np.ravel(self._samples["sigma"])[index]
        return sig ** 2, np.ravel(self._samples["mu"])[index], (self._samples["ar_roots"][index], self._samples["ma_coefs"][index])

    def _point_models(self, bestfit, npaths):
        sigsqr, mu, roots, ma = self._point_params(bestfit)
        return np.full(npaths, sigsqr), np.full(npaths, mu), (np.tile(roots, (npaths, 1)), np.tile(ma, (npaths, 1)))

    def _simulate_cond(self, sigsqr, mu, rest, time, seed):
        return carmcmcLib.simulate_cond_carma(self.time, self.y, self.ysig, sigsqr, rest[0], rest[1], mu, time, seed=seed)

    def simulate_paths(self, time, npaths=1, bestfit="random", seed=None, return_index=False):
        """`npaths` draws of the process at `time` conditional on the data -> [npaths][len(time)]: the ensemble the reference
        builds with `for i in range(nsim): ysim[i] = sample.simulate(time, bestfit='random')`, in two launches for all paths.
        bestfit 'random': every path under its own posterior sample; 'map', 'median', 'mean' or a sample index: that one
        model for all paths.  seed: the sample indices come from np.random.RandomState(seed) and the device generator is
        keyed by (seed, path), so a seed reproduces the ensemble; None: indices and a seed from numpy's global stream.
        return_index: also the sample index of every path (None unless bestfit is 'random')."""
        time = np.atleast_1d(np.asarray(time, dtype=float))
        npaths = int(npaths)
        rs = np.random if seed is None else np.random.RandomState(seed)
        index = None
        if bestfit == "random":
            index = rs.randint(0, self._samples["sigma"].shape[0], size=npaths)
            sigsqr, mu, rest = self._path_models(index)
        else:
            sigsqr, mu, rest = self._point_models(bestfit, npaths)
        dev_seed = int(np.random.randint(0, 2 ** 62)) if seed is None else int(seed)
        paths = self._simulate_cond(sigsqr, mu, rest, time, dev_seed)
        return (paths, index) if return_index else paths

    def predict(self, time, bestfit="map"):
        """Expected value and variance of the series at `time` given the data and a point estimate of
        the parameters (reference :755-805).  All times go to the GPU in one batched launch instead of
        one full re-filter per time.  Returns (yhat, yhat_var)."""
        scalar = np.isscalar(time)
        kf, mu = self.makeKalmanFilter(bestfit)
        m, v = kf.PredictBatch(np.atleast_1d(time))
        return (m[0] + mu, v[0]) if scalar else (m + mu, v)

    def smooth(self, time, bestfit="map"):
        """predict(time, bestfit) by the one-pass smoother: the same expected value and variance (to rounding) from ONE forward
        and ONE backward pass over the data and the requested times, O((n + M) p^2), where predict filters the series once per
        time, O(M n p^2).  predict stays the default, and for ONE model it is also the faster route on an MI355X at every M
        measured (tools/smooth_probe.py, profiles/smooth/README.md; CARMA(5,3), n = 270: 0.28 ms for any M <= 1000 against 0.6
        ms at M = 64, 2 ms at M = 1000 and 6 ms at M = 4000): its M filter runs are M lane groups side by side on an otherwise
        empty chip, the smoother is one wave's serial chain of 2 (n + M) steps.  The crossing lies where MANY models are smoothed
        at once -- predict_band, MultiContext.smooth, smooth_carma: with 256 models the smoother is ahead from M ~ 256 (2.5 x at M
        = 1000), with 1024 models at every M (2 x at M = 64, 6 x at M = 1000; n = 3000, M = 1000: 7 x).  The variance is returned
        as computed -- a difference that can come out <= 0 by rounding where ysig is tiny against the process.
        Returns (yhat, yhat_var)."""
        scalar = np.isscalar(time)
        kf, mu = self.makeKalmanFilter(bestfit)
        m, v = kf.SmoothBatch(np.atleast_1d(time))
        return (m[0] + mu, v[0]) if scalar else (m + mu, v)

    def _smooth_models(self, sigsqr, mu, rest, time, band):
        return carmcmcLib.smooth_carma(self.time, self.y, self.ysig, sigsqr, rest[0], rest[1], mu, time, band=band,
                                       return_singular=True)

    def predict_band(self, time, nsamples=None, seed=None, return_samples=False):
        """The interpolated light curve MARGINALISED over the posterior samples instead of under one point estimate: per time the
        mean and variance of the equal-weight mixture of the samples' predictive distributions,
            mean = (1/K) sum_k m_k,    var = (1/K) sum_k (v_k + (m_k - mean)^2),
        every sample smoothed in one pass and the mixture formed on the device (carma_smooth_*).  What the reference's users
        loop `sample.predict(time, bestfit=i)` for.  nsamples: use that many samples -- evenly spaced as plot_power_spectrum
        picks them, or, with a seed, drawn without replacement from np.random.RandomState(seed); None: all.  Samples with a
        repeated AR root are left out.  Returns (mean, var); return_samples: also the K x M means and variances of the samples
        and their indices."""
        time = np.atleast_1d(np.asarray(time, dtype=float))
        nall = self._samples["sigma"].shape[0]
        if seed is not None and nsamples is not None and nsamples < nall:
            index = np.sort(np.random.RandomState(seed).choice(nall, int(nsamples), replace=False))
        else:
            index = self._subsample(nsamples, nall)
        sigsqr, mu, rest = self._path_models(index)
        res = self._smooth_models(sigsqr, mu, rest, time, True if return_samples else "only")
        if return_samples:
            m, v, bm, bv, _ = res
            return bm, bv, m, v, index
        return res[0], res[1]

    def simulate(self, time, bestfit="map"):
        """Random draw of the process at `time` conditional on the data (reference :807-837)."""
        kf, mu = self.makeKalmanFilter(bestfit)
        return np.array(kf.Simulate(np.atleast_1d(time))) + mu

    def assess_fit(self, bestfit="map", nplot=256, doShow=False):
        """Numerical part of assess_fit (reference :687-753): the interpolated path on `nplot` times,
        the standardised residuals of the one-step predictions and their autocorrelation function.
        Plotting is outside the hot path."""
        kf, mu = self.makeKalmanFilter(bestfit)
        kf.Filter()
        kmean, kvar = np.array(kf.GetMean()), np.array(kf.GetVar())
        resid = (self.y - mu - kmean) / np.sqrt(kvar)
        tgrid = np.linspace(self.time.min(), self.time.max(), nplot)
        pm, pv = kf.PredictBatch(tgrid)
        r0 = resid - resid.mean()
        acf = np.correlate(r0, r0, mode="full")[r0.size - 1:] / np.sum(r0 * r0)
        return dict(time=tgrid, mean=pm + mu, var=pv, std_resid=resid, resid_acf=acf)


class Car1Sample(CarmaSample):
    """Samples of a CAR(1) model (reference :866-1035): theta = (sigma_y, scale, mu, ln omega)."""

    def __init__(self, time, y, ysig, sampler, filename=None):
        self.time, self.y, self.ysig, self.q, self.p = time, y, ysig, 0, 1
        self._sampler = sampler
        logpost = np.array(sampler.GetLogLikes())
        trace = np.array(sampler.getSamples())
        MCMCSample.__init__(self, logpost=logpost, trace=trace)
        self._samples["loglik"] = self._samples["logpost"] - np.array(
            [sampler.getLogPrior(carmcmcLib.vecD(row)) for row in trace])
        self.parameters = list(self._samples.keys())
        self.newaxis()
        self.mle = {}

    def generate_from_trace(self, trace):
        omega = np.exp(trace[:, 3])
        self._samples["var"] = trace[:, 0] ** 2
        self._samples["measerr_scale"] = trace[:, 1]
        self._samples["mu"] = trace[:, 2]
        self._samples["log_omega"] = trace[:, 3]
        self._samples["ar_roots"] = (-omega)[:, None] + 0j
        self._samples["psd_centroid"] = np.zeros((trace.shape[0], 1))
        self._samples["psd_width"] = omega[:, None] / (2.0 * np.pi)
        self._samples["ar_coefs"] = np.c_[np.ones_like(omega), omega]
        self._samples["ma_coefs"] = np.ones((trace.shape[0], 1))
        self._samples["sigma"] = np.sqrt(2.0 * omega * trace[:, 0] ** 2)

    def _point_params(self, bestfit):
        """(sigsqr, mu, log omega) of a point estimate (reference :925-948): 'map', 'median', anything else = posterior mean
        (of sigma^2, mu and log omega -- as the reference does); an integer picks one sample (as CarmaSample)."""
        sig, mu_s, lw = (np.ravel(self._samples[k]) for k in ("sigma", "mu", "log_omega"))
        if bestfit == "map":
            i = int(np.argmax(self._samples["logpost"]))
            sigsqr, mu, log_omega = sig[i] ** 2, mu_s[i], lw[i]
        elif bestfit == "median":
            sigsqr, mu, log_omega = np.median(sig) ** 2, np.median(mu_s), np.median(lw)
        elif isinstance(bestfit, (int, np.integer)):
            i = int(bestfit)
            sigsqr, mu, log_omega = sig[i] ** 2, mu_s[i], lw[i]
        else:
            sigsqr, mu, log_omega = np.mean(sig ** 2), np.mean(mu_s), np.mean(lw)
        return float(sigsqr), float(mu), float(log_omega)

    def makeKalmanFilter(self, bestfit):
        """KalmanFilter1 for a point estimate (_point_params; reference :925-948)."""
        sigsqr, mu, log_omega = self._point_params(bestfit)
        kf = carmcmcLib.KalmanFilter1(carmcmcLib.vecD(self.time), carmcmcLib.vecD(self.y - mu),
                                      carmcmcLib.vecD(self.ysig), sigsqr, float(np.exp(log_omega)))
        return kf, mu

    # simulate_paths is CarmaSample's, through this class's own parameter pick
    def _path_models(self, index):
        sig = np.ravel(self._samples["sigma"])[index]
        return sig ** 2, np.ravel(self._samples["mu"])[index], np.exp(np.ravel(self._samples["log_omega"])[index])

    def _point_models(self, bestfit, npaths):
        sigsqr, mu, log_omega = self._point_params(bestfit)
        return np.full(npaths, sigsqr), np.full(npaths, mu), np.full(npaths, float(np.exp(log_omega)))

    def _simulate_cond(self, sigsqr, mu, omega, time, seed):
        return carmcmcLib.simulate_cond_car1(self.time, self.y, self.ysig, sigsqr, omega, mu, time, seed=seed)

    def _smooth_models(self, sigsqr, mu, omega, time, band):
        return carmcmcLib.smooth_car1(self.time, self.y, self.ysig, sigsqr, omega, mu, time, band=band, return_singular=True)

    # (the spectrum sigma^2 / (omega^2 + (2 pi f)^2) of the reference (:1004-1013) is the general formula with
    # alpha(s) = s + omega, delta = 1 -- the arrays generate_from_trace stores -- so CarmaSample's device path serves it)


# ------------------------------------------------------------------------------------------------
def _vec(a):
    v = carmcmcLib.vecD()
    v.extend(np.asarray(a, dtype=float).tolist())
    return v


class CarmaModel(object):
    """Statistical inference with a CARMA(p,q) model (reference :12-192)."""

    def __init__(self, time, y, ysig, p=1, q=0):
        time, y, ysig = np.asarray(time, dtype=float), np.asarray(y, dtype=float), np.asarray(ysig, dtype=float)
        if not p > q:
            raise ValueError("Order of AR polynomial, p, must be larger than order of MA polynomial, q.")
        _, idx = np.unique(time, return_index=True)    # sorted, first occurrence of each time
        self.time, self.y, self.ysig = time[idx], y[idx], ysig[idx]
        self._time, self._y, self._ysig = _vec(self.time), _vec(self.y), _vec(self.ysig)
        self.p, self.q = p, q
        self.mcmc_sample = None

    def run_mcmc(self, nsamples, nburnin=None, ntemperatures=None, nthin=1, init=None, nreplicas=1, seed=None, dist=None):
        """Parallel-tempered RAM sampler on the GPU; defaults as the reference (:53-89):
        ntemperatures = max(10, p+q), nburnin = nsamples/2.  `dist`: an initialised torch.distributed module (one
        process per GPU, every rank makes the same call): the `nreplicas` independent ladders are split over the ranks
        and every rank returns the gathered samples of all of them (parallel.sharded_pt_run) -- the same arrays as the
        single-process call with the same seed."""
        nburnin, ntemperatures = _mcmc_defaults(nsamples, nburnin, ntemperatures, self.p, self.q)
        init = carmcmcLib.vecD() if init is None else _vec(init)
        if self.p == 1:
            cpp = carmcmcLib.run_mcmc_car1(nsamples, int(nburnin), self._time, self._y, self._ysig, nthin, init,
                                           nreplicas=nreplicas, seed=seed, dist=dist)
            sample = Car1Sample(self.time, self.y, self.ysig, cpp)
        else:
            cpp = carmcmcLib.run_mcmc_carma(nsamples, int(nburnin), self._time, self._y, self._ysig, self.p, self.q,
                                            ntemperatures, False, nthin, init, nreplicas=nreplicas, seed=seed, dist=dist)
            sample = CarmaSample(self.time, self.y, self.ysig, cpp, q=self.q)
        self.mcmc_sample = sample
        return sample

    # -- maximum likelihood ---------------------------------------------------------------------
    def _mle_bounds(self, p, q):
        """L-BFGS-B box of the reference (:219-240)."""
        return mle_bounds(self.time, self.y, p, q)

    def _mle_problem(self, p, q, ntrials, seed):
        """(model object, [ntrials, d] starting points, L-BFGS-B box) of a get_mle call (reference :195-240)."""
        if p == 1:
            proc = carmcmcLib.run_mcmc_car1(1, 25, self._time, self._y, self._ysig, 1, nreplicas=ntrials, seed=seed)
        else:
            proc = carmcmcLib.run_mcmc_carma(1, 25, self._time, self._y, self._ysig, p, q, 10, False, 1,
                                             nreplicas=ntrials, seed=seed)
            proc.SetMLE(True)
        bnds = self._mle_bounds(p, q)
        return proc, _clamp_starts(proc.getAllSamples()[0][:, 0, :].copy(), bnds, seed), bnds

    def get_mle(self, p, q, ntrials=100, njobs=1, seed=None, method="batched", return_all=False):
        """Best of `ntrials` bounded quasi-Newton fits started from short tempered MCMC runs
        (reference :92-129,195-260).  The reference launches ntrials separate 26-iteration samplers
        and calls the C++ log-density once per function evaluation; here ONE sampler call with
        `ntrials` independent replicas provides all starting points, and with method="batched" all
        starts are optimised in lock-step (carma_mle.hip, C ABI carma_mle_batched): one launch evaluates the
        finite-difference stencils of every start.  method="scipy" runs scipy's L-BFGS-B per start
        with a batched gradient.  `njobs` is accepted for compatibility.  Returns an object with
        .x, .fun (= -loglik), .message like scipy's OptimizeResult (return_all=True: the list of all ntrials results,
        in the order of the starts)."""
        proc, starts, bnds = self._mle_problem(p, q, ntrials, seed)
        d = starts.shape[1]

        if method == "batched":
            # the lock-step optimiser inside the library (carma_mle.hip): no interpreter between the launches
            results = _batch_results(*proc.minimizeBatch(starts, bnds))
            return results if return_all else _best_result(results)
        if method != "scipy":
            raise ValueError("method must be 'batched' or 'scipy'")

        def fun_and_grad(x):
            h = 1e-6 * np.maximum(1.0, np.abs(x))
            pts = np.tile(x, (2 * d + 1, 1))
            pts[1:d + 1] += np.diag(h)
            pts[d + 1:] -= np.diag(h)
            f = -np.asarray(proc.getLogDensityBatch(pts))
            fp, fm = f[1:d + 1], f[d + 1:]
            ok = np.isfinite(fp) & np.isfinite(fm)             # a stencil point outside the bounds is +inf: no inf - inf
            g = np.where(ok, np.where(ok, fp, 0.0) - np.where(ok, fm, 0.0), 0.0) / (2.0 * h)
            return (f[0] if np.isfinite(f[0]) else 1e300), g

        results = [minimize(fun_and_grad, x0, jac=True, method="L-BFGS-B", bounds=bnds) for x0 in starts]
        return results if return_all else min(results, key=lambda r: r.fun)

    def choose_order(self, pmax, qmax=None, pqlist=None, njobs=1, ntrials=100, seed=None, method="batched"):
        """Minimise AICc over a (p,q) grid (reference :131-192); sets self.p, self.q."""
        pqlist = _pq_grid(pmax, qmax, pqlist)
        # njobs (reference :131: processes of a multiprocessing pool, -1 = all cores): here THREADS, each driving its own
        # orders -- every order has its own context and stream, the library calls release the interpreter lock, and the
        # launches of one order (a few thousand evaluations) leave most of the chip to the others
        nthreads = (os.cpu_count() or 1) if njobs is not None and njobs < 0 else max(1, int(njobs or 1))
        if nthreads > 1 and len(pqlist) > 1:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=min(nthreads, len(pqlist))) as pool:
                MLEs = list(pool.map(lambda pq: self.get_mle(pq[0], pq[1], ntrials=ntrials, seed=seed, method=method), pqlist))
        else:
            MLEs = [self.get_mle(p, q, ntrials=ntrials, njobs=njobs, seed=seed, method=method) for p, q in pqlist]
        best, AICc, order = _choose_order(MLEs, pqlist, self.time.size)
        if order is not None:
            self.p, self.q = order
        return best, pqlist, AICc


# ------------------------------------------------------------------------------------------------
class CarmaModelSet(object):
    """Many light curves, each fitted on its own (no counterpart in the reference, which wraps one series per CarmaModel):
    get_mle / choose_order of every series with all series' starts optimised together in ONE lock-step run on a
    multi-series context (MultiContext, carma_mle_batched_ms).  series: a list of (time, y, ysig); each becomes a
    CarmaModel (self.models), so its data are sorted and deduplicated as CarmaModel does."""

    def __init__(self, series, p=1, q=0):
        series = list(series)
        if not series:
            raise ValueError("CarmaModelSet needs at least one series")
        if not p > q:
            raise ValueError("Order of AR polynomial, p, must be larger than order of MA polynomial, q.")
        self.models = []
        for s, item in enumerate(series):
            t, y, e = _series_item(item, "series", s)
            if np.unique(t).size < 2:
                raise ValueError("series %d has fewer than 2 distinct times" % s)
            self.models.append(CarmaModel(t, y, e, p=p, q=q))
        self.p, self.q = p, q
        self.nseries = len(self.models)
        self._mctx = {}
        self.timing = {}
        self.mcmc_samples = None

    def context(self, p, q):
        """The MultiContext of order (p, q) over every series (created once; the prior bound max_stdev of the samplers that
        get_mle's objective carries, carmcmc.cpp:35-40,85-89)."""
        key = (int(p), int(q))
        if key not in self._mctx:
            from ._lib import MultiContext
            self._mctx[key] = MultiContext([(m.time, m.y, m.ysig) for m in self.models], key[0], key[1],
                                           max_stdev=[carmcmcLib._pop_max_stdev(m.y) for m in self.models])
        return self._mctx[key]

    def loglik(self, theta, which):
        """-f of get_mle's objective: the log-density with the prior bounds of the MLE (SetMLE(true) for p > 1) of theta[i]
        on series which[i], every row in one launch."""
        theta = np.asarray(theta, dtype=float)
        rows = np.atleast_2d(theta)
        w = _which(which, rows.shape[0], self.nseries, "series")
        out = self.context(self.p, self.q).logdensity(rows, w, ignore_prior=self.p > 1)
        return float(out[0]) if theta.ndim == 1 else out

    def run_mcmc(self, nsamples, nburnin=None, ntemperatures=None, nthin=1, init=None, nreplicas=1, seed=None):
        """CarmaModel.run_mcmc of EVERY series in one sampler run (MultiContext.pt_run): all series' ladders advance in the
        same launches, one chain per lane.  Defaults as CarmaModel.run_mcmc: ntemperatures = max(10, p + q) (p = 1: one
        chain at temperature 1), nburnin = nsamples / 2.  init: None or [S, d], row s for series s.  Returns a list of S
        CarmaSample (p = 1: Car1Sample) in the caller's order, also kept as self.mcmc_samples and models[s].mcmc_sample."""
        p, q, S = self.p, self.q, self.nseries
        d = 4 if p == 1 else 3 + p + q
        nsamples, nburnin, ntemperatures, nthin, nreplicas = _mcmc_args(nsamples, nburnin, ntemperatures, nthin, nreplicas, p, q)
        if p == 1:
            ntemperatures = 1
        if init is not None:
            init = np.asarray(init, dtype=float)
            if init.shape != (S, d):
                raise ValueError("init must be [%d, %d] (one row per series), got %r" % (S, d, init.shape))
        mc = self.context(p, q)
        # longest series first: the ladders that share a wave then have similar lengths
        order = np.argsort(-np.asarray(mc.n), kind="stable")
        samples, logposts = mc.pt_run(order, ntemperatures, nreplicas, nsamples, nburnin, nthin,
                                      init=None if init is None else init[order], seed=carmcmcLib._seed(seed))
        acc, swp = mc.pt_stats()
        # the "loglik" column (prior bounds ignored) of all series' traces: one launch
        loglik = None
        if p > 1:
            ns = samples.shape[2]
            loglik = mc.logdensity(samples[:, 0].reshape(-1, d), np.repeat(order, ns), ignore_prior=True).reshape(S, ns)
        # and the "sigma" column: the samples of all series back to back, one launch (one lane per sample)
        sigma = [None] * S
        if p > 1:
            ins = [CarmaSample._sigma_inputs_of(samples[j, 0], p, q) for j in range(S)]
            flat = carmcmcLib.sigma_noise_batch(*(np.concatenate([a[k] for a in ins]) for k in range(3)))
            sigma = [ins[j] + (flat[j * ns:(j + 1) * ns],) for j in range(S)]
        out = [None] * S
        for j, s in enumerate(order):
            m = self.models[s]
            run = carmcmcLib.SetRunSampler(mc, s, samples[j], logposts[j], None if loglik is None else loglik[j], acc[j], swp[j],
                                           sigma=sigma[j])
            out[s] = Car1Sample(m.time, m.y, m.ysig, run) if p == 1 else CarmaSample(m.time, m.y, m.ysig, run, q=q)
            m.mcmc_sample = out[s]
        self.mcmc_samples = out
        return out

    def power_spectrum_band(self, percentile=68.0, nsamples=None, freq=None, samples=None):
        """CarmaSample.power_spectrum_band of EVERY series in one call per order present (carma_mpsd_band): the posterior median
        and `percentile` credibility band of the power spectrum.  samples: a list of S CarmaSample / Car1Sample, by default
        self.mcmc_samples of run_mcmc.  freq: None (each series' own 1000 log-spaced frequencies), one grid for all series, or
        [S, nf].  nsamples: the evenly spaced subsample of each series that the single-series call takes.  Returns
        (lower, upper, median, frequencies), each [S, nf]."""
        S = self.nseries
        samples = _resolve_samples(samples, self.mcmc_samples, S)
        if freq is None:
            freq = np.stack([smp._psd_frequencies() for smp in samples])
        else:
            freq = np.asarray(freq, dtype=float)
            if freq.ndim == 1:
                freq = np.broadcast_to(freq, (S, freq.size))
            if freq.ndim != 2 or freq.shape[0] != S or freq.shape[1] < 1:
                raise ValueError("freq must be [nf] or [%d, nf], got %r" % (S, freq.shape))
        lower = (100.0 - percentile) / 2.0
        ins = []
        for smp in samples:
            index = smp._subsample(nsamples, smp._samples["sigma"].shape[0])
            ins.append(smp._psd_inputs(index))
        band = np.empty((S, freq.shape[1], 3))
        for _, idx in group_by_order([(a.shape[1], m.shape[1]) for a, m, _ in ins]).items():
            start = np.zeros(len(idx) + 1, dtype=np.int64)
            start[1:] = np.cumsum([ins[s][2].size for s in idx])
            band[idx] = carmcmcLib.mpsd_band(*(np.concatenate([ins[s][k] for s in idx]) for k in range(3)), start, freq[idx],
                                             [lower, 50.0, 100.0 - lower])
        return band[:, :, 0], band[:, :, 2], band[:, :, 1], np.array(freq)

    def diagnostics(self, samples=None):
        """CarmaSample.diagnostics of EVERY series, in the caller's order, in two device calls (carma_chain_diag: one over the
        parameter vectors of all series' replicas, one over their log-posteriors): tau [S, R, d + 1], ess [S, d + 1],
        rhat [S, d + 1], status [S, R, d + 1], mean and sigma [S, R, d + 1]; the last column is logpost.  samples: a list of S
        CarmaSample / Car1Sample, by default self.mcmc_samples of run_mcmc; all must hold the same number of replicas, of
        samples and of parameters."""
        S = self.nseries
        samples = _resolve_samples(samples, self.mcmc_samples, S)
        runs = [smp._sampler.getAllSamples() for smp in samples]
        if any(par is None or lp is None for par, lp in runs):
            raise ValueError("a sample object's sampler holds no samples")
        shape = np.shape(runs[0][0])
        for s, (par, lp) in enumerate(runs):
            if len(np.shape(par)) != 3 or np.shape(par) != shape or np.shape(lp) != shape[:2]:
                raise ValueError("series %d: samples of shape %r with log-posteriors %r; every series must hold [R, L, d] = %r "
                                 "(the same replicas, sample count and order)" % (s, np.shape(par), np.shape(lp), tuple(shape)))
        par = np.stack([np.asarray(r[0], dtype=float) for r in runs])
        lp = np.stack([np.asarray(r[1], dtype=float) for r in runs])[..., None]
        out = _diagnostics_of(carmcmcLib.chain_diag(par), carmcmcLib.chain_diag(lp))
        out["ess"] = _ess_of(out["tau"], out["status"], shape[1])
        return out

    def _set_starts(self, p, q, ntrials, seed):
        """The starts of get_mle(starts="set"): CarmaModel._mle_problem's short tempered run (25 adapting iterations, one
        sample, 10 temperatures -- 1 for p = 1 -- ntrials replicas) of ALL series as one multi-series run, then the same
        post-processing per series."""
        mc = self.context(p, q)
        order = np.argsort(-np.asarray(mc.n), kind="stable")
        samples, _ = mc.pt_run(order, 1 if p == 1 else 10, int(ntrials), 1, 25, 1, seed=carmcmcLib._seed(seed))
        starts = np.empty((self.nseries, int(ntrials), mc.d))
        starts[order] = samples[:, :, 0, :]
        for s, m in enumerate(self.models):
            _clamp_starts(starts[s], m._mle_bounds(p, q), seed)
        return starts

    def get_mle(self, p, q, ntrials=100, seed=None, starts=None, return_all=False):
        """CarmaModel.get_mle of every series.  starts None: each series' starts drawn exactly as CarmaModel.get_mle draws
        them (a short tempered sampler run per series, same seed); "set": all series' starts from ONE multi-series sampler
        run with the same arguments (other draws than None gives -- the chains' random streams are keyed by their place in
        the set's ensemble); else an array [S, ntrials, d].  All S x ntrials starts are then optimised in ONE lock-step run.
        Returns a list of S BatchResult (return_all: S lists of ntrials).  self.timing holds the seconds spent drawing
        starts and optimising."""
        if not p > q:
            raise ValueError("Order of AR polynomial, p, must be larger than order of MA polynomial, q.")
        if isinstance(starts, str) and starts != "set":
            raise ValueError("starts must be None, 'set' or an array [S, ntrials, d], got %r" % starts)
        S = self.nseries
        t0 = perf_counter()
        if starts is None:
            starts = np.stack([m._mle_problem(p, q, ntrials, seed)[1] for m in self.models])
        elif isinstance(starts, str):
            starts = self._set_starts(p, q, ntrials, seed)
        else:
            starts = np.asarray(starts, dtype=float)
            d = 4 if p == 1 else 3 + p + q
            if starts.ndim != 3 or starts.shape[0] != S or starts.shape[2] != d:
                raise ValueError("starts must be [%d, ntrials, %d], got %r" % (S, d, starts.shape))
        t1 = perf_counter()
        nt, d = starts.shape[1], starts.shape[2]
        lo, hi = (np.stack(a) for a in zip(*[_bounds_lohi(m._mle_bounds(p, q)) for m in self.models]))
        which = np.repeat(np.arange(S), nt)
        res = self.context(p, q).mle_batched(starts.reshape(S * nt, d), which, lo[which], hi[which], ignore_prior=p > 1)
        self.timing = _timing(t0, t1, perf_counter())
        return _results_per_member(res, S, nt, return_all)

    def choose_order(self, pmax, qmax=None, pqlist=None, ntrials=100, seed=None):
        """CarmaModel.choose_order of every series: one get_mle over the whole set per order, AICc with each series' own n.
        Returns a list of S (best, pqlist, AICc) triples; self.orders holds each series' chosen (p, q)."""
        pqlist = _pq_grid(pmax, qmax, pqlist)
        MLEs = [self.get_mle(p, q, ntrials=ntrials, seed=seed) for p, q in pqlist]
        out, self.orders = [], []
        for s, m in enumerate(self.models):
            best, AICc, order = _choose_order([mles[s] for mles in MLEs], pqlist, m.time.size)
            out.append((best, pqlist, AICc))
            self.orders.append(order or pqlist[0])
        return out

    def _fit_items(self, fits, orders):
        """Per-order work lists of predict / assess_fit: {(p, q): (series indices, sigsqr, roots, ma, mu)}.  fits: S results
        (anything with .x, or the vectors themselves); orders: None (self.orders of choose_order, else (self.p, self.q) for all),
        one (p, q), or one per series.  Everything is checked here, before any library call."""
        fits = list(fits)
        if len(fits) != self.nseries:
            raise ValueError("fits must hold one result per series (%d), got %d" % (self.nseries, len(fits)))
        if orders is None:
            orders = getattr(self, "orders", None) or [(self.p, self.q)] * self.nseries
        orders = [tuple(o) for o in np.asarray(orders, dtype=int).reshape(-1, 2)]
        if len(orders) == 1:
            orders = orders * self.nseries
        if len(orders) != self.nseries:
            raise ValueError("orders must hold one (p, q) per series (%d), got %d" % (self.nseries, len(orders)))
        items = {}
        for (p, q), idx in group_by_order(orders).items():
            if not p > q >= 0:
                raise ValueError("Order of AR polynomial, p, must be larger than order of MA polynomial, q.")
            mods = []
            for s in idx:
                try:
                    mods.append(mle_to_model(getattr(fits[s], "x", fits[s]), p, q))
                except ValueError as err:
                    raise ValueError("series %d: %s" % (s, err))
            ma = np.zeros((len(idx), max(q + 1, 1)))
            for k, m in enumerate(mods):
                ma[k, :m[2].size] = m[2]
            items[(p, q)] = (np.array(idx), np.array([m[0] for m in mods]), np.array([m[1] for m in mods]), ma,
                             np.array([m[3] for m in mods]))
        return items

    def _at_times(self, method, times, fits, orders):
        """predict / smooth: `method` of every order's context at its series' times."""
        tlist = _times_per_row(times, self.nseries)
        if len(tlist) != self.nseries:
            raise ValueError("times must be one array, or one per series (%d), got %d" % (self.nseries, len(tlist)))
        mean, var = [None] * self.nseries, [None] * self.nseries
        for (p, q), (idx, sig, roots, ma, mu) in self._fit_items(fits, orders).items():
            pm, pv = getattr(self.context(p, q), method)(idx, sig, roots, ma, [tlist[s] for s in idx], mu=mu)
            for k, s in enumerate(idx):
                mean[s], var[s] = pm[k], pv[k]
        return mean, var

    def predict(self, times, fits, orders=None):
        """CarmaSample.predict of every series at its fitted model: expected value and variance at `times` -- one array for
        every series, or one per series (a list of S arrays, or an array [S, M]) -- given the series' data.  fits: S results as
        get_mle returns them (or the best of each choose_order triple); orders: see _fit_items.  The series are grouped by order,
        one launch per order present.  Returns two lists of S arrays."""
        return self._at_times("predict", times, fits, orders)

    def smooth(self, times, fits, orders=None):
        """predict(times, fits, orders) by the one-pass smoother (CarmaSample.smooth of every series at its fitted model;
        MultiContext.smooth): arguments and return values as predict, one call per order present."""
        return self._at_times("smooth", times, fits, orders)

    def assess_fit(self, fits, orders=None, nplot=256):
        """CarmaSample.assess_fit of every series at its fitted model: a list of S dicts with the interpolated path on `nplot`
        times (time, mean, var), the standardised residuals of the one-step predictions (std_resid) and their autocorrelation
        function (resid_acf).  One filter launch and one predict launch per order present."""
        out = [None] * self.nseries
        for (p, q), (idx, sig, roots, ma, mu) in self._fit_items(fits, orders).items():
            ctx = self.context(p, q)
            kmean, kvar, sing = ctx.kfilter(idx, sig, roots, ma, mu=mu)
            if sing.any():
                raise carmcmcLib._lib.CarmaError("KalmanFilterp: singular eigenvector matrix (solve failed) for series %s"
                                            % idx[sing][:8].tolist())
            grids = [np.linspace(self.models[s].time.min(), self.models[s].time.max(), nplot) for s in idx]
            pm, pv = ctx.predict(idx, sig, roots, ma, grids, mu=mu)
            for k, s in enumerate(idx):
                resid = (self.models[s].y - kmean[k]) / np.sqrt(kvar[k])
                r0 = resid - resid.mean()
                acf = np.correlate(r0, r0, mode="full")[r0.size - 1:]
                acf = acf / acf[0]                            # (by its own lag 0, not np.sum(r0 * r0): resid_acf[0] is exactly 1)
                out[s] = dict(time=grids[k], mean=pm[k], var=pv[k], std_resid=resid, resid_acf=acf)
        return out


# ------------------------------------------------------------------------------------------------
class CarmaBandsModel(object):
    """ONE CARMA(p,q) process observed in several bands with a lag between them (no counterpart in the reference): several
    filters of a survey, the images of a lensed quasar, the continuum and a delayed line of a reverberation campaign.  Band
    b sees  y = a_b x(t - lag_b) + mu_b + noise;  band 0 is the reference band (lag 0, a = 1, mu = theta[2]).

    bands: a list of (time, y, ysig), each sorted and deduplicated as CarmaModel does; lag_bounds: one (lo, hi) pair for each
    band after the first (one pair alone for two bands): the box of that band's lag; None: +- half the time all bands span.
    The parameter vector is CarmaModel's (ysigma, measerr_scale, mu, log-quadratic AR parameters, MA parameters) followed
    by (lag_b, log a_b, mu_b) for b = 1 ... K - 1.  Every log-density is one lane of k_logdens_carma_mband, which merges the
    bands in the order that vector's lags give."""

    def __init__(self, bands, p=1, q=0, lag_bounds=None):
        bands = list(bands)
        if not bands:
            raise ValueError("CarmaBandsModel needs at least one band")
        if not p > q:
            raise ValueError("Order of AR polynomial, p, must be larger than order of MA polynomial, q.")
        self.bands = []
        for b, item in enumerate(bands):
            t, y, e = _series_item(item, "band", b, least=1)
            _, idx = np.unique(t, return_index=True)         # sorted, first occurrence of each time
            self.bands.append((t[idx], y[idx], e[idx]))
        self.K = len(self.bands)
        self.p, self.q = int(p), int(q)
        self.d = 3 + self.p + self.q
        self.dx = self.d + 3 * (self.K - 1)
        if lag_bounds is None:
            span = max(t.max() for t, _, _ in self.bands) - min(t.min() for t, _, _ in self.bands)
            lag_bounds = [(-0.5 * span, 0.5 * span)] * (self.K - 1)
        self.lag_bounds = np.asarray(lag_bounds, dtype=float).reshape(-1, 2)
        if self.lag_bounds.shape[0] != self.K - 1:
            raise ValueError("lag_bounds must hold one (lo, hi) pair for each band after the first")
        self._ctx = None
        self.mcmc_sample = None

    def context(self):
        """The BandsContext of the model (created once; max_stdev as the samplers that provide get_mle's starts set it)."""
        if self._ctx is None:
            from ._lib import BandsContext
            self._ctx = BandsContext(self.bands, self.p, self.q, lag_bounds=self.lag_bounds,
                                     max_stdev=carmcmcLib._pop_max_stdev(self.bands[0][1]))
        return self._ctx

    def _lag_cols(self):
        return self.d + 3 * np.arange(self.K - 1)

    def loglik(self, theta):
        """-f of get_mle's objective: the log-density of the extended vector(s) with the prior bounds of the MLE (SetMLE(true)
        for p > 1: neither the CARMA bounds nor the lag boxes are tested).  theta: [dx] or [B, dx], one launch."""
        return self.context().logdensity(theta, ignore_prior=self.p > 1)

    def logpost(self, theta):
        """The log-posterior: -inf outside the prior bounds of the CARMA part (band 0's) or a lag box."""
        return self.context().logdensity(theta, ignore_prior=False)

    def _starts(self, ntrials, seed):
        """([ntrials, dx] starts, lo [dx], hi [dx]): the CARMA part as CarmaModel._mle_problem draws it on band 0, lags
        uniform in their boxes, log a_b = log(std y_b / std y_0), mu_b = mean y_b."""
        t0, y0, e0 = self.bands[0]
        _, st, bnds = CarmaModel(t0, y0, e0, p=self.p, q=self.q)._mle_problem(self.p, self.q, ntrials, seed)
        return (self._extend_starts(st, seed),) + self._box(bnds)

    def _box(self, bnds):
        """(lo [dx], hi [dx]) of the optimiser: the box bnds of band 0's CarmaModel, the band columns unbounded (the lags stay in
        their boxes inside the library)."""
        return _bounds_lohi(bnds + [(None, None)] * (3 * (self.K - 1)))

    def _extend_starts(self, st, seed):
        """_starts behind its CARMA part st [ntrials, d]: the band columns."""
        y0 = self.bands[0][1]
        rng = np.random.default_rng(seed)
        x0 = np.empty((st.shape[0], self.dx))
        x0[:, :self.d] = st
        s0 = y0.std()
        for b in range(1, self.K):
            yb = self.bands[b][1]
            c = self.d + 3 * (b - 1)
            x0[:, c] = rng.uniform(self.lag_bounds[b - 1, 0], self.lag_bounds[b - 1, 1], st.shape[0])
            x0[:, c + 1] = np.log(yb.std() / s0) if yb.std() > 0 and s0 > 0 else 0.0
            x0[:, c + 2] = yb.mean()
        return x0

    def get_mle(self, ntrials=100, seed=None, return_all=False):
        """Best of `ntrials` bounded quasi-Newton fits of the extended vector, all advanced in lock-step
        (carma_bands_mle_batched); the lags stay inside their boxes.  Returns an object with .x, .fun (= -loglik), .message
        (return_all: the list of all ntrials results, in the order of the starts)."""
        x0, lo, hi = self._starts(ntrials, seed)
        results = _batch_results(*self.context().mle_batched(x0, lo, hi, ignore_prior=self.p > 1))
        return results if return_all else _best_result(results)

    def lag_profile(self, lags, ntrials=8, seed=None):
        """The profile log-likelihood over the lags: at each of the L rows of `lags` ([L] for two bands, else [L, K - 1]) the
        other parameters are optimised from `ntrials` starts with the lags held fixed -- all L x ntrials starts in ONE
        lock-step run.  Returns (loglik [L], x [L, dx]): the best log-likelihood at each row and the optimum that reaches it,
        whose lag entries are the given lags unchanged."""
        if self.K < 2:
            raise ValueError("lag_profile needs at least two bands")
        lags = _lag_grid(lags, self.K, self.lag_bounds)
        L = lags.shape[0]
        x0, lo, hi = self._starts(ntrials, seed)
        nt = x0.shape[0]
        fixed = np.repeat(lags, nt, axis=0)
        xs, fs, nits, nfevs, sts = self.context().mle_batched(np.tile(x0, (L, 1)), lo, hi, fixed_lag=fixed,
                                                              ignore_prior=self.p > 1)
        return _profile_best(fs, xs, L, nt)

    def _smooth_rows(self, theta, time, band, moments):
        out = self.context().smooth(theta, band, time, moments=moments)
        inv = np.atleast_1d(out[-1])
        if inv.any():
            raise ValueError("CarmaBandsModel.smooth: row %d has a repeated AR root or a non-finite lag, scale or offset"
                             % int(np.argmax(inv)))
        return out[:-1]

    def smooth(self, theta, time, band=0):
        """The interpolated light curve of band `band`: mean and variance of a_b x(t - lag_b) + mu_b at the observer times `time`
        [M] given all data of all bands (carma_bands_smooth; no prior, the semantics of loglik).  theta: [dx] -> (mean [M],
        var [M]); [B, dx] -> ([B, M], [B, M]), every row on the merge order its own lags give, one launch.  ValueError on an
        invalid row."""
        return self._smooth_rows(theta, time, band, False)

    def smooth_band(self, thetas, time, band=0):
        """(band_mean [M], band_var [M]): the moment-matched equal-weight mixture of smooth() over the rows of thetas [B, dx] --
        the optima of a lag_profile, of get_mle(return_all=True), or whatever vectors the caller holds.  Mixed on the device."""
        return self._smooth_rows(thetas, time, band, True)[2:]

    def run_mcmc(self, nsamples, nburnin=None, ntemperatures=None, nthin=1, init=None, nreplicas=1, seed=None, scale_bounds=None,
                 offset_bounds=None):
        """Parallel-tempered RAM sampler on the extended vector (carma_bands_pt_run): the posterior of the lags, scales and
        offsets together with the CARMA part.  Defaults as CarmaModel.run_mcmc: nburnin = nsamples / 2, ntemperatures =
        max(10, p + q); nreplicas independent ladders advance in the same launches, one chain per lane.  init: None or [dx], the
        starting value of every chain where its log-posterior is finite.
        logpost is flat in log a_b and mu_b and tends to a constant as a_b -> 0, so the sampler keeps both in a box:
        scale_bounds = [K - 1] pairs (lo, hi) of a_b, offset_bounds = [K - 1] pairs of mu_b; None: a_b within a factor 1000 of
        std y_b / std y_0, mu_b within the range of y_b widened by its span on either side.
        Returns a CarmaBandsSample (all replicas' cold-chain draws), kept as mcmc_sample."""
        if self.K < 1:
            raise ValueError("run_mcmc needs at least one band")
        nsamples, nburnin, ntemperatures, nthin, nreplicas = _mcmc_args(nsamples, nburnin, ntemperatures, nthin, nreplicas,
                                                                        self.p, self.q)
        if init is not None:
            init = np.asarray(init, dtype=float)
            if init.shape != (self.dx,):
                raise ValueError("init must be [%d], got %r" % (self.dx, init.shape))
        sb = _band_bounds("scale_bounds", scale_bounds, self.K, positive=True)
        ob = _band_bounds("offset_bounds", offset_bounds, self.K)
        ctx = self.context()
        samples, logposts = ctx.pt_run(ntemperatures, nreplicas, nsamples, nburnin, nthin, init, carmcmcLib._seed(seed),
                                       band_box=_sampler_box(ctx.pt_default_box(), sb, ob))
        self.mcmc_sample = CarmaBandsSample(self, samples, logposts)
        return self.mcmc_sample

    def merged(self, theta):
        """The single light curve the bands make at theta, in the units of band 0: (time, y, ysig, band) with
        time = t - lag_b, y = (y_b - mu_b) / a_b + mu_0, ysig = ysig_b / a_b, sorted by time (equal times: the lower band
        first), band = the band each datum came from.  Host numpy.  CarmaModel(time, y, ysig, p, q) on it gives the sampler and
        the power spectrum at the fitted lag -- but CarmaModel DROPS data with equal times (it keeps the first of each), which
        the multi-band likelihood keeps.  For the interpolated light curve of a band use smooth / smooth_band: they keep every
        datum, work in that band's units and take many vectors with different lags per call."""
        theta = np.asarray(theta, dtype=float).reshape(self.dx)
        ts, ys, es, bs = [], [], [], []
        for b, (t, y, e) in enumerate(self.bands):
            if b == 0:
                lag, a, mu = 0.0, 1.0, theta[2]
            else:
                c = self.d + 3 * (b - 1)
                lag, a, mu = theta[c], np.exp(theta[c + 1]), theta[c + 2]
            ts.append(t - lag)
            ys.append((y - mu) / a + theta[2])
            es.append(e / a)
            bs.append(np.full(t.size, b, dtype=np.int64))
        t, y, e, band = (np.concatenate(a) for a in (ts, ys, es, bs))
        order = np.lexsort((band, t))
        return t[order], y[order], e[order], band[order]


class CarmaBandsSet(object):
    """Many multi-band objects, each fitted on its own: the AGN of a survey field seen in the same K filters, the systems of a
    lens-monitoring campaign.  get_mle / lag_profile of every object with the starts of ALL objects optimised together in ONE
    lock-step run on a set context (BandsSetContext, carma_bandset_mle_batched): every optimiser step is one launch for the whole
    set, and an object's results are those of its own CarmaBandsModel, bit for bit.

    objects: a list of S lists of K (time, y, ysig) -- every object in the same K bands (one that lacks a band belongs to
    another set); each becomes a CarmaBandsModel (self.models).  lag_bounds: None (each object's default), one list of K - 1
    (lo, hi) pairs for all objects, or a list of S such lists."""

    def __init__(self, objects, p=1, q=0, lag_bounds=None):
        objects = [list(o) for o in objects]
        if not objects:
            raise ValueError("CarmaBandsSet needs at least one object")
        K = len(objects[0])
        for s, o in enumerate(objects):
            if len(o) != K:
                raise ValueError("object %d has %d bands, object 0 has %d: the objects of a set share their bands" % (s, len(o), K))
        S = len(objects)
        if lag_bounds is None:
            lbs = [None] * S
        else:
            lb = np.asarray(lag_bounds, dtype=float)
            if lb.size == 2 * (K - 1) and lb.ndim <= 2:
                lbs = [lb.reshape(K - 1, 2)] * S
            elif lb.size == 2 * S * (K - 1):
                lbs = list(lb.reshape(S, K - 1, 2))
            else:
                raise ValueError("lag_bounds must hold %d (lo, hi) pair(s), for all objects or for each of the %d objects"
                                 % (K - 1, S))
        self.models = []
        for s, o in enumerate(objects):
            try:
                self.models.append(CarmaBandsModel(o, p=p, q=q, lag_bounds=lbs[s]))
            except ValueError as ex:
                raise ValueError("object %d: %s" % (s, ex))
        self.p, self.q, self.K, self.nobjects = int(p), int(q), K, S
        self.d, self.dx = self.models[0].d, self.models[0].dx
        self._ctx = None
        self.timing = {}

    def context(self):
        """The BandsSetContext over every object (created once; lag boxes and max_stdev as each CarmaBandsModel.context() has
        them)."""
        if self._ctx is None:
            from ._lib import BandsSetContext
            self._ctx = BandsSetContext([m.bands for m in self.models], self.p, self.q,
                                        lag_bounds=np.stack([m.lag_bounds for m in self.models]),
                                        max_stdev=[carmcmcLib._pop_max_stdev(m.bands[0][1]) for m in self.models])
        return self._ctx

    def _logdensity(self, theta, which, ignore_prior):
        theta = np.asarray(theta, dtype=float)
        rows = np.atleast_2d(theta)
        w = _which(which, rows.shape[0], self.nobjects, "object")
        out = self.context().logdensity(rows, w, ignore_prior=ignore_prior)
        return float(out[0]) if theta.ndim == 1 else out

    def loglik(self, theta, which):
        """CarmaBandsModel.loglik of theta[i] on object which[i] (one index per row, or one for all), every row in one launch."""
        return self._logdensity(theta, which, self.p > 1)

    def logpost(self, theta, which):
        """CarmaBandsModel.logpost of theta[i] on object which[i], every row in one launch."""
        return self._logdensity(theta, which, False)

    def _boxes(self):
        """(lo, hi) [S, dx]: each object's optimiser box, as CarmaBandsModel._starts gives it."""
        boxes = [m._box(mle_bounds(m.bands[0][0], m.bands[0][1], self.p, self.q)) for m in self.models]
        return tuple(np.stack(a) for a in zip(*boxes))

    def get_mle(self, ntrials=100, seed=None, starts=None, return_all=False):
        """CarmaBandsModel.get_mle of every object.  starts None: each object's starts drawn exactly as its CarmaBandsModel
        draws them (same seed); "set": the CARMA part of all objects' starts from ONE multi-series sampler run over the
        objects' band 0 (CarmaModelSet's starts="set"; other draws than None gives), the band columns drawn as for None; else
        an array [S, ntrials, dx].  All S x ntrials starts are then optimised in ONE lock-step run.  Returns a list of S results
        (return_all: S lists of ntrials).  self.timing holds the seconds spent drawing starts and optimising.  smooth() takes
        the list this returns and draws every object's interpolated light curves in its K bands, in one call."""
        if isinstance(starts, str) and starts != "set":
            raise ValueError("starts must be None, 'set' or an array [S, ntrials, dx], got %r" % starts)
        S = self.nobjects
        t0 = perf_counter()
        if starts is None:
            starts = np.stack([m._starts(ntrials, seed)[0] for m in self.models])
        elif isinstance(starts, str):
            band0 = CarmaModelSet([m.bands[0] for m in self.models], p=self.p, q=self.q)
            carma = band0._set_starts(self.p, self.q, ntrials, seed)
            starts = np.stack([m._extend_starts(carma[s], seed) for s, m in enumerate(self.models)])
        else:
            starts = np.asarray(starts, dtype=float)
            if starts.ndim != 3 or starts.shape[0] != S or starts.shape[2] != self.dx:
                raise ValueError("starts must be [%d, ntrials, %d], got %r" % (S, self.dx, starts.shape))
        lo, hi = self._boxes()
        t1 = perf_counter()
        nt = starts.shape[1]
        which = np.repeat(np.arange(S), nt)
        res = self.context().mle_batched(starts.reshape(S * nt, self.dx), which, lo[which], hi[which], ignore_prior=self.p > 1)
        self.timing = _timing(t0, t1, perf_counter())
        return _results_per_member(res, S, nt, return_all)

    def _lag_grids(self, lags):
        """lags of lag_profile -> S arrays [L_s, K - 1], each checked against its object's boxes.  One grid for all objects
        ([L] for two bands, else [L, K - 1]), or a list (not an array) of S grids."""
        K, S = self.K, self.nobjects
        per = isinstance(lags, (list, tuple)) and len(lags) == S and all(np.ndim(g) >= (1 if K == 2 else 2) for g in lags)
        return [_lag_grid(g, K, self.models[s].lag_bounds, obj=s) for s, g in enumerate(lags if per else [lags] * S)]

    def lag_profile(self, lags, ntrials=8, seed=None):
        """CarmaBandsModel.lag_profile of every object: `lags` is one grid for all objects or a list of one grid per object;
        all S x L x ntrials starts run in ONE lock-step call.  Returns a list of S (loglik [L], x [L, dx])."""
        if self.K < 2:
            raise ValueError("lag_profile needs at least two bands")
        grids = self._lag_grids(lags)
        t0 = perf_counter()
        x0s, los, his, fixed, which = [], [], [], [], []
        for s, (m, g) in enumerate(zip(self.models, grids)):
            x0, lo, hi = m._starts(ntrials, seed)
            nt, L = x0.shape[0], g.shape[0]
            x0s.append(np.tile(x0, (L, 1)))
            los.append(np.tile(lo, (L * nt, 1)))
            his.append(np.tile(hi, (L * nt, 1)))
            fixed.append(np.repeat(g, nt, axis=0))
            which.append(np.full(L * nt, s))
        t1 = perf_counter()
        xs, fs, nits, nfevs, sts = self.context().mle_batched(np.concatenate(x0s), np.concatenate(which), np.concatenate(los),
                                                              np.concatenate(his), fixed_lag=np.concatenate(fixed),
                                                              ignore_prior=self.p > 1)
        self.timing = _timing(t0, t1, perf_counter())
        out, k = [], 0
        for g in grids:
            L, nt = g.shape[0], x0s[len(out)].shape[0] // g.shape[0]
            out.append(_profile_best(fs[k:k + L * nt], xs[k:k + L * nt], L, nt))
            k += L * nt
        return out

    def smooth(self, thetas, time, band=None):
        """CarmaBandsModel.smooth of every object, in ONE call for all objects, bands and rows (carma_bandset_smooth).  thetas: a
        list of S entries, one per object: a vector [dx], an array [B_s, dx] or an object with .x (what get_mle returns); time:
        one array for all objects, or one per object -- a list of S arrays or an array [S, M]; any other count is a ValueError; band: None (all K bands), an int or a list of bands.  Returns a list of
        S (mean, var), arrays [nbands, B_s, M_s] -- without the row axis where the entry was a single vector, without the band
        axis where band is an int; every entry has the bits of models[s].smooth(theta, time, band=b).  ValueError on an invalid
        row, named by object and row."""
        S = self.nobjects
        thetas = list(thetas)
        if len(thetas) != S:
            raise ValueError("thetas must hold one entry per object (%d), got %d" % (S, len(thetas)))
        times = [np.atleast_1d(np.asarray(t, dtype=float)).ravel() for t in _times_per_row(time, S)]
        if len(times) != S:
            raise ValueError("time must be one array, or one per object (%d), got %d" % (S, len(times)))
        bands = list(range(self.K)) if band is None else [int(b) for b in np.atleast_1d(band)]
        rows, which, bo, tl, ones = [], [], [], [], []
        for s, th in enumerate(thetas):
            x = np.asarray(getattr(th, "x", th), dtype=float)
            if x.ndim > 2 or x.shape[-1] != self.dx:
                raise ValueError("object %d: thetas must be [%d] or [B, %d], got %r" % (s, self.dx, self.dx, x.shape))
            ones.append(x.ndim == 1)
            x = x.reshape(-1, self.dx)
            for b in bands:
                rows.append(x)
                which += [s] * x.shape[0]
                bo += [b] * x.shape[0]
                tl += [times[s]] * x.shape[0]
        means, variances, inv = self.context().smooth(np.concatenate(rows), which, bo, tl, return_invalid=True)
        if inv.any():
            i = int(np.argmax(inv))
            s, n = which[i], rows[which[i] * len(bands)].shape[0]
            raise ValueError("CarmaBandsSet.smooth: object %d, row %d has a repeated AR root or a non-finite lag, scale or offset"
                             % (s, (i - which.index(s)) % n))
        out, k = [], 0
        for s in range(S):
            n = rows[s * len(bands)].shape[0]
            shape = (len(bands), n, times[s].size)
            pair = [np.array(a[k:k + len(bands) * n]).reshape(shape) for a in (means, variances)]
            k += len(bands) * n
            if ones[s]:
                pair = [a[:, 0] for a in pair]
            if band is not None and np.ndim(band) == 0:
                pair = [a[0] for a in pair]
            out.append(tuple(pair))
        return out

    def _run_bounds(self, which, name, bounds, positive=False):
        """scale_bounds / offset_bounds of run_mcmc -> a list of len(which) entries, None or [K - 1, 2], each checked
        (_band_bounds): None, one [K - 1, 2] for all objects, or [len(which), K - 1, 2]."""
        if bounds is None:
            return [None] * len(which)
        a = np.asarray(bounds, dtype=float)
        if a.ndim == 2:
            a = np.broadcast_to(a, (len(which),) + a.shape)
        if a.ndim != 3 or a.shape[0] != len(which):
            raise ValueError("%s must be [%d, 2] for all objects or [%d, %d, 2], one per object, got shape %r"
                             % (name, self.K - 1, len(which), self.K - 1, a.shape))
        out = []
        for i, s in enumerate(which):
            try:
                out.append(_band_bounds(name, a[i], self.K, positive))
            except ValueError as ex:
                raise ValueError("object %d: %s" % (s, ex))
        return out

    def run_mcmc(self, nsamples, nburnin=None, ntemperatures=None, nthin=1, init=None, nreplicas=1, seed=None, scale_bounds=None,
                 offset_bounds=None, which=None):
        """CarmaBandsModel.run_mcmc of the objects `which` (None: every object) in ONE sampler run (BandsSetContext.pt_run,
        carma_bandset_pt_run): the ladders of all objects advance in the same launches, one chain per lane, a wave on one object.
        Defaults as CarmaBandsModel.run_mcmc: nburnin = nsamples / 2, ntemperatures = max(10, p + q).  init: None, [dx] for all
        objects or [len(which), dx]; scale_bounds / offset_bounds: None (each object's default box), [K - 1, 2] for all objects or
        [len(which), K - 1, 2].  The default ladder fills 10 of a wave's 64 lanes: nreplicas fills the rest at no cost in time.
        Returns a list of CarmaBandsSample, one per entry of `which` in the caller's order, each also kept as that model's
        mcmc_sample."""
        nsamples, nburnin, ntemperatures, nthin, nreplicas = _mcmc_args(nsamples, nburnin, ntemperatures, nthin, nreplicas,
                                                                        self.p, self.q)
        if which is None:
            which = np.arange(self.nobjects)
        which = np.asarray(which)
        if which.ndim != 1 or which.size < 1 or which.dtype.kind not in "iu":
            raise ValueError("which must be a list of at least one object index")
        if which.min() < 0 or which.max() >= self.nobjects:
            raise ValueError("which: object index out of range [0, %d)" % self.nobjects)
        which = which.astype(np.int64)
        M = which.size
        if init is not None:
            init = np.asarray(init, dtype=float)
            if init.shape == (self.dx,):
                init = np.broadcast_to(init, (M, self.dx))
            if init.shape != (M, self.dx):
                raise ValueError("init must be [%d] or [%d, %d] (one row per object of which), got %r" % (self.dx, M, self.dx, init.shape))
        sbs = self._run_bounds(which, "scale_bounds", scale_bounds, positive=True)
        obs = self._run_bounds(which, "offset_bounds", offset_bounds)
        ctx = self.context()
        lo, hi = np.empty((M, self.K - 1, 2)), np.empty((M, self.K - 1, 2))
        for i, s in enumerate(which):
            lo[i], hi[i] = _sampler_box(ctx.pt_default_box(s), sbs[i], obs[i])
        # longest object first: the waves in flight together then have similar trip counts
        order = np.argsort(-ctx.n.sum(axis=1)[which], kind="stable")
        runs = which[order]
        samples, logposts = ctx.pt_run(runs, ntemperatures, nreplicas, nsamples, nburnin, nthin,
                                       init=None if init is None else init[order], seed=carmcmcLib._seed(seed),
                                       band_box=(lo[order], hi[order]))
        # the "loglik" column (prior bounds ignored) of all objects' draws: one launch; the "sigma" column: one more
        per = samples.shape[1] * samples.shape[2]
        flat = samples.reshape(-1, self.dx)
        loglik = ctx.logdensity(flat, np.repeat(runs, per), ignore_prior=True).reshape(M, per)
        sigma = carmcmcLib.sigma_noise_batch(*CarmaSample._sigma_inputs_of(flat[:, :self.d], self.p, self.q)).reshape(M, per)
        out = [None] * M
        for j, i in enumerate(order):
            m = self.models[which[i]]
            out[i] = CarmaBandsSample(m, samples[j], logposts[j], loglik=loglik[j], sigma=sigma[j])
            m.mcmc_sample = out[i]
        return out


class CarmaBandsSample(MCMCSample):
    """The draws of CarmaBandsModel.run_mcmc: every replica's cold chain, replica after replica, n = R x nsamples rows.

    `_samples` holds the entries CarmaSample derives from the CARMA part (the first d columns: var, measerr_scale, mu,
    quad_coefs, ar_roots, psd_centroid, psd_width, ar_coefs, ma_coefs, sigma), the band terms lag, log_scale, scale = a_b and
    offset = mu_b ([n, K - 1] each), logpost, and loglik (the log-density with the prior bounds ignored, one batched launch).
    samples: [R, nsamples, dx]; logposts: [R, nsamples].  loglik [n] and sigma [n] may be given by whoever holds them already;
    without them they come from the device.  There is no predict or simulate: smooth_band interpolates a band."""

    def __init__(self, model, samples, logposts, loglik=None, sigma=None):
        samples, logposts = np.asarray(samples, dtype=float), np.asarray(logposts, dtype=float)
        if samples.ndim != 3 or samples.shape[2] != model.dx or logposts.shape != samples.shape[:2]:
            raise ValueError("CarmaBandsSample: samples must be [R, n, %d] and logposts [R, n], got %r and %r"
                             % (model.dx, samples.shape, logposts.shape))
        self.model, self.p, self.q, self.K = model, model.p, model.q, model.K
        self.time, self.y, self.ysig = model.bands[0]
        self._all = samples, logposts
        trace = samples.reshape(-1, model.dx)
        self.trace = trace
        d = model.d
        super(CarmaBandsSample, self).__init__(logpost=logposts.ravel())
        # the CARMA part, by CarmaSample's own steps on the first d columns
        CarmaSample.generate_from_trace(self, trace[:, :d])
        CarmaSample._ar_roots(self)
        CarmaSample._ar_coefs(self)
        self._samples["ma_coefs"] = CarmaSample._ma_coefs_of(trace[:, :d], self.p, self.q)
        if sigma is None:
            sigma = carmcmcLib.sigma_noise_batch(self._samples["ar_roots"], self._samples["ma_coefs"], self._samples["var"])
        self._samples["sigma"] = np.asarray(sigma, dtype=float).reshape(trace.shape[0])
        cols = d + 3 * np.arange(model.K - 1)
        self._samples["lag"] = trace[:, cols]
        self._samples["log_scale"] = trace[:, cols + 1]
        self._samples["scale"] = np.exp(trace[:, cols + 1])
        self._samples["offset"] = trace[:, cols + 2]
        if loglik is None:
            loglik = model.context().logdensity(trace, ignore_prior=True)
        self._samples["loglik"] = np.asarray(loglik, dtype=float).reshape(trace.shape[0])
        self.parameters = list(self._samples.keys())
        self.newaxis()

    def lag_summary(self, percentile=68.0):
        """(median, lower, upper) of every band's lag, [K - 1] each: the central `percentile` per cent interval."""
        lower = (100.0 - percentile) / 2.0
        med, lo, hi = np.percentile(self._samples["lag"], [50.0, lower, 100.0 - lower], axis=0)
        return med, lo, hi

    def smooth_band(self, time, band=0, nsamples=None, seed=None):
        """(band_mean [M], band_var [M]) of band `band` at the observer times `time`: CarmaBandsModel.smooth_band over a subsample
        of the draws (all of them by default; nsamples: evenly spaced ones, or drawn without replacement with a seed), so the
        band is marginalised over the posterior of the lags as well."""
        n = self.trace.shape[0]
        if seed is not None and nsamples is not None and nsamples < n:
            index = np.sort(np.random.default_rng(seed).choice(n, int(nsamples), replace=False))
        else:
            index = CarmaSample._subsample(nsamples, n)
        return self.model.smooth_band(self.trace[index], time, band=band)

    def diagnostics(self):
        """As CarmaSample.diagnostics, over all replicas and the dx columns of the extended vector followed by logpost: tau
        [R, dx + 1], ess [dx + 1], rhat [dx + 1], status, mean, sigma [R, dx + 1] (carma_chain_diag, in column groups of at most
        carma_chain_diag_dmax() columns)."""
        samples, logposts = self._all
        dmax = carmcmcLib.chain_diag_dmax()
        parts = [carmcmcLib.chain_diag(np.ascontiguousarray(samples[None, :, :, c:c + dmax]))
                 for c in range(0, samples.shape[2], dmax)]
        par = {k: np.concatenate([p[k] for p in parts], axis=-1) for k in ("tau", "mean", "sigma", "status", "rhat")}
        out = _diagnostics_of(par, carmcmcLib.chain_diag(logposts[None, :, :, None]))
        out = {k: v[0] for k, v in out.items()}
        out["ess"] = _ess_of(out["tau"], out["status"], samples.shape[1])
        return out

    # the power spectrum of the CARMA part: CarmaSample's steps on the entries above (carma_psd_band)
    _subsample = staticmethod(CarmaSample._subsample)
    _psd_frequencies = CarmaSample._psd_frequencies
    _psd_inputs = CarmaSample._psd_inputs
    _psd_credint = CarmaSample._psd_credint
    power_spectrum_band = CarmaSample.power_spectrum_band
