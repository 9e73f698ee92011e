"""The power-spectrum band of a whole sampled set in one call (CarmaModelSet.power_spectrum_band, carma_mpsd_band) against the
loop it replaces, [s.power_spectrum_band(68.0) for s in samples].  One JSON line per case on stdout (and appended to the file
MPOST_PROBE_OUT names, when it is set):
  set64, set1024   S CARMA(5,3) series with 200 samples each, every series' own 1000 frequencies
  set16x5000       16 series with 5000 samples each
  ragged           64 series with 50 .. 5000 samples (log-uniform)
  limit            ONE series of 1024, 4096 and carma_mpsd_fused_max() samples: the set call (fused kernel) against
                   _lib.psd_band (grid to HBM + row selection), to place the fused limit
The sample objects are CarmaSample built from prior-like parameter vectors (no sampler run: the band does not care where the
samples came from).  The loop is timed on MPOST_PROBE_LOOP_S series spread over the set and scaled to S (stated in the line).
Times are host wall-clock around calls that end in a synchronise, median of MPOST_PROBE_REPS after a warm-up, every copy
included on both sides."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import carma_pack_amd as cpa  # noqa: E402
from carma_pack_amd import _lib  # noqa: E402
from carma_pack_amd.carma_pack import CarmaSample  # noqa: E402
from carma_pack_amd.synth import irregular_series, theta_batch  # noqa: E402

REPS = int(os.environ.get("MPOST_PROBE_REPS", "3"))
LOOP_S = int(os.environ.get("MPOST_PROBE_LOOP_S", "128"))
OUT = os.environ.get("MPOST_PROBE_OUT")
P, Q = 5, 3


def timed(fn, reps=REPS):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def emit(rec):
    rec.update(_lib.build_ids())
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "a") as f:
            f.write(line + "\n")


class Stored(object):
    """A sampler object that holds a trace (what CarmaSample wraps); the log-densities play no part in the band."""

    def __init__(self, theta):
        self._theta = theta

    def getSamples(self):
        return self._theta.tolist()

    def GetLogLikes(self):
        return [0.0] * self._theta.shape[0]

    def SetMLE(self, flag):
        pass

    def getLogDensityBatch(self, thetas):
        return np.zeros(len(thetas))


def sample_objects(series, counts, seed):
    rng = np.random.default_rng(seed)
    out = []
    for (t, y, e), ns in zip(series, counts):
        base = theta_batch(rng, min(int(ns), 256), P, Q, t, y)
        out.append(CarmaSample(t, y, e, Stored(base[rng.integers(0, base.shape[0], int(ns))]), q=Q))
    return out


def set_case(name, counts, seed):
    S = len(counts)
    series = [irregular_series(270, seed=seed + s) for s in range(S)]
    mset = cpa.CarmaModelSet(series, P, Q)
    samples = sample_objects(series, counts, seed)
    s_med, s_lo, s_hi = timed(lambda: mset.power_spectrum_band(68.0, samples=samples))
    rec = dict(case=name, p=P, q=Q, nseries=S, ns_min=int(min(counts)), ns_max=int(max(counts)), nfreq=1000,
               fused_max=_lib.mpsd_fused_max(), set_s=s_med, set_min_s=s_lo, set_max_s=s_hi)
    L = min(LOOP_S, S)
    if L > 0:
        pick = np.linspace(0, S - 1, L).astype(int)
        l_med, l_lo, l_hi = timed(lambda: [samples[s].power_spectrum_band(68.0) for s in pick])
        got = mset.power_spectrum_band(68.0, samples=samples)
        same = all(np.allclose(got[2][s], samples[s].power_spectrum_band(68.0)[2], rtol=4e-16, atol=0.0) for s in pick[:4])
        rec.update(loop_series_timed=L, loop_s_scaled=l_med * S / L,
                   loop_min_s_scaled=l_lo * S / L, loop_max_s_scaled=l_hi * S / L, speedup=l_med * S / L / s_med, same=bool(same))
    emit(rec)


def limit_case(seed=7):
    t, y, e = irregular_series(270, seed=seed)
    freq = np.exp(np.linspace(np.log(1e-3), np.log(0.5), 1000))
    pcs = [16.0, 50.0, 84.0]
    for ns in (1024, 4096, _lib.mpsd_fused_max()):
        smp = sample_objects([(t, y, e)], [ns], seed)[0]
        ar, ma, sig = smp._psd_inputs(np.arange(ns))
        f = timed(lambda: _lib.mpsd_band(ar, ma, sig, [0, ns], freq, pcs))
        g = timed(lambda: _lib.psd_band(ar, ma, sig, freq, pcs))
        emit(dict(case="limit", ns=ns, nfreq=1000, fused_s=f[0], fused_min_s=f[1], grid_s=g[0], grid_min_s=g[1],
                  grid_over_fused=g[0] / f[0]))


def ragged_counts(S, seed):
    return np.exp(np.random.default_rng(seed).uniform(np.log(50.0), np.log(5000.0), S)).astype(int)


CASES = {"set64": lambda: set_case("set64", [200] * 64, 100), "set1024": lambda: set_case("set1024", [200] * 1024, 200),
         "set16x5000": lambda: set_case("set16x5000", [5000] * 16, 300), "ragged": lambda: set_case("ragged", ragged_counts(64, 9), 400),
         "limit": limit_case}

if __name__ == "__main__":
    assert _lib.lib.carma_device_count() >= 1, "mpost_probe needs a GPU"
    for c in sys.argv[1:] or list(CASES):
        CASES[c]()
