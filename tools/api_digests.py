"""SHA-256 digests of what the four model classes return, for holding a change of the Python layer to the bits of its parent.

  python tools/api_digests.py          one line per (class, order, method) on stdout (appended to the file API_DIGESTS_OUT names,
                                       when set): run_mcmc and get_mle of CarmaModel, CarmaModelSet, CarmaBandsModel and
                                       CarmaBandsSet, and lag_profile and smooth of the two band classes.

Fixed seeds and the smallest shapes: two series of 12 and 9 data; two objects of K = 2 bands (12 + 9 and 9 + 12 data); orders
(1, 0) and (2, 1); ntrials = 3, nsamples = 8, nreplicas = 2, ntemperatures = 3.  A digest covers every array a call returns: of
a sample object every entry of `_samples` in the order of its keys and the replicas' draws, of a fit x, fun, nit, nfev, success
and message.  A few seconds on one MI355X; the lines of two runs are equal when the two trees compute the same bits
(profiles/mband/api_digests.txt)."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.environ.get("API_DIGESTS_OUT")
NTRIALS, NSAMPLES, NREPLICAS, NTEMPS, SEED = 3, 8, 2, 3, 11


def feed(h, x):
    """Everything a call returned, into the hash: containers by their entries, arrays by dtype, shape and bytes."""
    if isinstance(x, (list, tuple)):
        h.update(b"[%d" % len(x))
        for v in x:
            feed(h, v)
    elif isinstance(x, dict):
        for k in sorted(x):
            h.update(str(k).encode())
            feed(h, x[k])
    elif hasattr(x, "_samples"):                                # a sample object
        feed(h, x._samples)
        feed(h, x._all if hasattr(x, "_all") else x._sampler.getAllSamples())
    elif hasattr(x, "nfev"):                                    # a fit
        feed(h, [x.x, x.fun, x.nit, x.nfev, bool(x.success), str(x.message)])
    elif isinstance(x, str):
        h.update(x.encode())
    else:
        a = np.ascontiguousarray(x)
        h.update(("%s%r" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())


def emit(label, x):
    h = hashlib.sha256()
    feed(h, x)
    line = "%-44s %s" % (label, h.hexdigest())
    print(line, flush=True)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "a") as f:
            f.write(line + "\n")


def main():
    import carma_pack_amd as cpa
    from carma_pack_amd.synth import irregular_series
    assert cpa._lib.lib.carma_device_count() >= 1, "api_digests needs a GPU"
    series = [irregular_series(12, seed=3), irregular_series(9, seed=4)]
    objects = [[series[0], (series[1][0] + 0.4, 2.0 * series[1][1] + 1.0, series[1][2])],
               [series[1], (series[0][0] - 0.3, 0.5 * series[0][1] - 1.0, series[0][2])]]
    mcmc = dict(nburnin=6, ntemperatures=NTEMPS, nreplicas=NREPLICAS, seed=SEED)
    lags = np.array([-1.0, 0.0, 1.5])
    times = np.array([2.5, 0.5, 7.25])
    for p, q in ((1, 0), (2, 1)):
        tag = "(%d,%d)" % (p, q)
        m = cpa.CarmaModel(*series[0], p=p, q=q)
        emit("CarmaModel%s.run_mcmc" % tag, m.run_mcmc(NSAMPLES, **mcmc))
        emit("CarmaModel%s.get_mle" % tag, m.get_mle(p, q, ntrials=NTRIALS, seed=SEED))
        emit("CarmaModel%s.get_mle(return_all)" % tag, m.get_mle(p, q, ntrials=NTRIALS, seed=SEED, return_all=True))
        ms = cpa.CarmaModelSet(series, p=p, q=q)
        emit("CarmaModelSet%s.run_mcmc" % tag, ms.run_mcmc(NSAMPLES, **mcmc))
        for starts in (None, "set"):
            emit("CarmaModelSet%s.get_mle(starts=%r)" % (tag, starts), ms.get_mle(p, q, ntrials=NTRIALS, seed=SEED, starts=starts))
        emit("CarmaModelSet%s.get_mle(return_all)" % tag, ms.get_mle(p, q, ntrials=NTRIALS, seed=SEED, return_all=True))
        bm = cpa.CarmaBandsModel(objects[0], p=p, q=q, lag_bounds=[(-2.0, 2.0)])
        emit("CarmaBandsModel%s.run_mcmc" % tag, bm.run_mcmc(NSAMPLES, **mcmc))
        emit("CarmaBandsModel%s.run_mcmc(boxes)" % tag,
             bm.run_mcmc(NSAMPLES, scale_bounds=[(0.1, 10.0)], offset_bounds=[(-100.0, 100.0)], **mcmc))
        fit = bm.get_mle(ntrials=NTRIALS, seed=SEED)
        emit("CarmaBandsModel%s.get_mle" % tag, fit)
        emit("CarmaBandsModel%s.get_mle(return_all)" % tag, bm.get_mle(ntrials=NTRIALS, seed=SEED, return_all=True))
        prof = bm.lag_profile(lags, ntrials=NTRIALS, seed=SEED)
        emit("CarmaBandsModel%s.lag_profile" % tag, prof)
        emit("CarmaBandsModel%s.smooth" % tag, [bm.smooth(fit.x, times, band=b) for b in (0, 1)] + [bm.smooth(prof[1], times, band=1)])
        emit("CarmaBandsModel%s.smooth_band" % tag, bm.smooth_band(prof[1], times, band=1))
        bs = cpa.CarmaBandsSet(objects, p=p, q=q, lag_bounds=[(-2.0, 2.0)])
        emit("CarmaBandsSet%s.run_mcmc" % tag, bs.run_mcmc(NSAMPLES, **mcmc))
        emit("CarmaBandsSet%s.run_mcmc(which, boxes)" % tag,
             bs.run_mcmc(NSAMPLES, which=[1, 0], scale_bounds=[[(0.1, 10.0)], [(0.2, 5.0)]], offset_bounds=[(-100.0, 100.0)], **mcmc))
        fits = None
        for starts in (None, "set"):
            fits = bs.get_mle(ntrials=NTRIALS, seed=SEED, starts=starts)
            emit("CarmaBandsSet%s.get_mle(starts=%r)" % (tag, starts), fits)
        emit("CarmaBandsSet%s.get_mle(return_all)" % tag, bs.get_mle(ntrials=NTRIALS, seed=SEED, return_all=True))
        profs = bs.lag_profile([lags, lags[:2]], ntrials=NTRIALS, seed=SEED)
        emit("CarmaBandsSet%s.lag_profile" % tag, profs)
        emit("CarmaBandsSet%s.smooth" % tag, [bs.smooth(fits, times), bs.smooth([pr[1] for pr in profs], [times, times[:2]], band=1)])


if __name__ == "__main__":
    main()
