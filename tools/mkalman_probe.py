"""Filter and predict of a whole set in one launch (carma_mkfilter / carma_mpredict) against a loop over KalmanHandle objects.
One JSON line per case on stdout (and appended to the file MKALMAN_PROBE_OUT names, when it is set):
  equal    S = 4096 CARMA(5,3) series of n = 270, one model each: MultiContext.kfilter, .predict at 256 times per series
  ragged   the same with n log-uniform in 50 .. 5000
Times are host wall-clock around calls that end in a stream synchronise, median of REPS after a warm-up, all copies included on
both sides.  The loop builds a KalmanHandle per series (allocation, upload of the series), calls filter() / predict() and drops
it -- what a pipeline without the set calls does; it is timed on LOOP_S series and scaled to S (stated in the line).  The line
also holds the log-density call on the same items (the same recursion without the 2 n stores).  Kernel times: run under
rocprofv3 --kernel-trace --stats with MKALMAN_PROBE_LOOP_S=0 (no loop)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import carma_pack_amd as cpa  # noqa: E402
from carma_pack_amd.carma_pack import mle_to_model  # noqa: E402
from carma_pack_amd.synth import irregular_series, theta_batch  # noqa: E402

REPS = int(os.environ.get("MKALMAN_PROBE_REPS", "5"))
LOOP_S = int(os.environ.get("MKALMAN_PROBE_LOOP_S", "512"))
OUT = os.environ.get("MKALMAN_PROBE_OUT")
NT = 256


def timed(fn, reps=REPS):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def emit(rec):
    rec.update(cpa._lib.build_ids())
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "a") as f:
            f.write(line + "\n")


def case(name, p, q, lengths, seed):
    S = len(lengths)
    series = [irregular_series(int(n), seed=seed + s) for s, n in enumerate(lengths)]
    mc = cpa.MultiContext(series, p, q)
    rng = np.random.default_rng(seed)
    th = np.concatenate([theta_batch(rng, 1, p, q, t, y) for t, y, _ in series])
    mods = [mle_to_model(x, p, q) for x in th]
    sig, roots = np.array([m[0] for m in mods]), np.array([m[1] for m in mods])
    ma, mu = np.array([m[2] for m in mods]), np.array([m[3] for m in mods])
    which = np.arange(S)
    times = [np.linspace(t[0] - 5.0, t[-1] + 5.0, NT) for t, _, _ in series]
    points = float(mc.n.sum())
    f_med, f_lo, f_hi = timed(lambda: mc.kfilter(which, sig, roots, ma, mu=mu))
    p_med, p_lo, p_hi = timed(lambda: mc.predict(which, sig, roots, ma, times, mu=mu))
    l_med, _, _ = timed(lambda: mc.logdensity(th, which, ignore_prior=True))
    rec = dict(case=name, p=p, q=q, nseries=S, n_min=int(mc.n.min()), n_max=int(mc.n.max()), n_mean=float(mc.n.mean()),
               times_per_series=NT, kfilter_s=f_med, kfilter_min_s=f_lo, kfilter_max_s=f_hi, kfilter_points_per_s=points / f_med,
               predict_s=p_med, predict_min_s=p_lo, predict_max_s=p_hi, predict_times_per_s=S * NT / p_med,
               logdensity_same_items_s=l_med)
    L = min(LOOP_S, S)
    if L > 0:
        def loop_filter():
            for s in range(L):
                t, y, e = series[s]
                cpa._lib.KalmanHandle(t, y - mu[s], e, sig[s], roots[s], ma[s]).filter()

        def loop_predict():
            for s in range(L):
                t, y, e = series[s]
                cpa._lib.KalmanHandle(t, y - mu[s], e, sig[s], roots[s], ma[s]).predict(times[s])
        lf, _, _ = timed(loop_filter, reps=max(1, REPS // 2))
        lp, _, _ = timed(loop_predict, reps=max(1, REPS // 2))
        rec.update(loop_series_timed=L, loop_kfilter_s=lf * S / L, loop_predict_s=lp * S / L,
                   kfilter_speedup_vs_loop=(lf * S / L) / f_med, predict_speedup_vs_loop=(lp * S / L) / p_med)
    emit(rec)


def main():
    assert cpa._lib.lib.carma_device_count() >= 1, "mkalman_probe needs a GPU"
    which = sys.argv[1:] or ["equal", "ragged"]
    if "equal" in which:
        case("equal", 5, 3, [270] * 4096, 10000)
    if "ragged" in which:
        n = np.exp(np.random.default_rng(5).uniform(np.log(50), np.log(5000), 4096)).astype(int)
        case("ragged", 5, 3, n, 20000)


if __name__ == "__main__":
    main()
