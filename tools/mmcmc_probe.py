"""The sampler over many series (CarmaModelSet.run_mcmc, carma_mpt_*) against what it replaces.  One JSON line per case on stdout
(and appended to the file MMCMC_PROBE_OUT names, when it is set):
  set64, set1024   CarmaModelSet.run_mcmc on S CARMA(5,3) series of n = 270 (T = 10, R = 1) against a loop over CarmaModel.run_mcmc
                   with identical arguments; the loop is timed on MMCMC_PROBE_LOOP_S series and scaled to S (stated in the line)
  ragged           the same with n log-uniform in 50 .. 5000
  k1               the sampler's log-density kernel alone (MultiContext.pt_logdensity, copies included on both sides) against the
                   wave-per-series kernel (MultiContext.logdensity) on the same vectors at R T = 64, where a wave is one series in
                   both: per-lane vector loads against scalar loads of the records
  k1sort           the sampler's kernel at T = 10 on ragged lengths, runs sorted longest first against the caller's order
  mle              CarmaModelSet.get_mle on 1000 CAR(1) series: the timing split with starts="set" against the default
Times are host wall-clock around calls that end in a stream synchronise, median of MMCMC_PROBE_REPS after a warm-up.  Kernel
times: run a case under rocprofv3 --kernel-trace --stats with MMCMC_PROBE_LOOP_S=0 (no loop), in a run of its own."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import carma_pack_amd as cpa  # noqa: E402
from carma_pack_amd.synth import irregular_series, theta_batch  # noqa: E402

REPS = int(os.environ.get("MMCMC_PROBE_REPS", "3"))
LOOP_S = int(os.environ.get("MMCMC_PROBE_LOOP_S", "32"))
OUT = os.environ.get("MMCMC_PROBE_OUT")
NSAMPLES, NBURN = int(os.environ.get("MMCMC_PROBE_NSAMPLES", "200")), int(os.environ.get("MMCMC_PROBE_NBURN", "100"))


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


def ragged_lengths(S, seed):
    return np.exp(np.random.default_rng(seed).uniform(np.log(50.0), np.log(5000.0), S)).astype(int)


def run_case(name, lengths, seed):
    p, q, S = 5, 3, len(lengths)
    series = [irregular_series(int(n), seed=seed + s) for s, n in enumerate(lengths)]
    mset = cpa.CarmaModelSet(series, p, q)
    mset.context(p, q)                                        # (the upload of the set is not part of either side)
    s_med, s_lo, s_hi = timed(lambda: mset.run_mcmc(NSAMPLES, nburnin=NBURN, seed=1))
    iters = NBURN + NSAMPLES
    rec = dict(case=name, p=p, q=q, nseries=S, n_min=int(min(lengths)), n_max=int(max(lengths)), ntemperatures=10, nreplicas=1,
               iterations=iters, set_s=s_med, set_min_s=s_lo, set_max_s=s_hi, set_us_per_iteration=1e6 * s_med / iters)
    L = min(LOOP_S, S)
    if L > 0:
        pick = np.linspace(0, S - 1, L).astype(int)           # across the lengths
        models = [cpa.CarmaModel(*series[s], p=p, q=q) for s in pick]
        l_med, l_lo, l_hi = timed(lambda: [m.run_mcmc(NSAMPLES, nburnin=NBURN, seed=1) for m in models], reps=max(1, REPS - 1))
        rec.update(loop_series_timed=L, loop_s_scaled=l_med * S / L, loop_min_s_scaled=l_lo * S / L, loop_max_s_scaled=l_hi * S / L,
                   speedup=l_med * S / L / s_med)
    emit(rec)


def k1_case(seed=5):
    p, q, S = 5, 3, 1024
    series = [irregular_series(270, seed=seed + s) for s in range(S)]
    mc = cpa.MultiContext(series, p, q)
    rng = np.random.default_rng(seed)
    mc.pt_create(np.arange(S), 64, 1, 5)
    th = np.stack([theta_batch(rng, 64, p, q, t, y) for t, y, _ in series])
    which = np.repeat(np.arange(S), 64)
    a = timed(lambda: mc.pt_logdensity(th))
    b = timed(lambda: mc.logdensity(th.reshape(-1, mc.d), which))
    same = bool(np.array_equal(mc.pt_logdensity(th).ravel(), mc.logdensity(th.reshape(-1, mc.d), which), equal_nan=True))
    emit(dict(case="k1", p=p, q=q, nseries=S, n=270, chains=S * 64, chain_per_lane_s=a[0], chain_per_lane_min_s=a[1],
              wave_per_series_s=b[0], wave_per_series_min_s=b[1], same_bits=same))


def k1sort_case(seed=6):
    p, q, S, T = 5, 3, 1024, 10
    lengths = ragged_lengths(S, seed)
    series = [irregular_series(int(n), seed=seed + s) for s, n in enumerate(lengths)]
    mc = cpa.MultiContext(series, p, q)
    rng = np.random.default_rng(seed)
    th = np.stack([theta_batch(rng, T, p, q, t, y) for t, y, _ in series])
    order = np.argsort(-mc.n, kind="stable")
    mc.pt_create(order, T, 1, 5)
    a = timed(lambda: mc.pt_logdensity(th[order]))
    mc.pt_create(np.arange(S), T, 1, 5)
    b = timed(lambda: mc.pt_logdensity(th))
    emit(dict(case="k1sort", p=p, q=q, nseries=S, n_min=int(lengths.min()), n_max=int(lengths.max()), ntemperatures=T,
              sorted_s=a[0], sorted_min_s=a[1], unsorted_s=b[0], unsorted_min_s=b[1]))


def mle_case(seed=7):
    S = int(os.environ.get("MMCMC_PROBE_MLE_S", "1000"))
    series = [irregular_series(270, seed=seed + s) for s in range(S)]
    mset = cpa.CarmaModelSet(series, 1, 0)
    mset.context(1, 0)
    rec = dict(case="mle", p=1, q=0, nseries=S, n=270, ntrials=8)
    for name, starts in (("set", "set"), ("default", None)):
        t0 = time.perf_counter()
        best = mset.get_mle(1, 0, ntrials=8, seed=3, starts=starts)
        rec[name + "_total_s"] = time.perf_counter() - t0
        rec[name + "_starts_s"], rec[name + "_optimise_s"] = mset.timing["starts_s"], mset.timing["optimise_s"]
        rec[name + "_median_fun"] = float(np.median([r.fun for r in best]))
    emit(rec)


CASES = {"set64": lambda: run_case("set64", [270] * 64, 100), "set1024": lambda: run_case("set1024", [270] * 1024, 200),
         "ragged": lambda: run_case("ragged", ragged_lengths(int(os.environ.get("MMCMC_PROBE_RAGGED_S", "256")), 9), 300),
         "k1": k1_case, "k1sort": k1sort_case, "mle": mle_case}

if __name__ == "__main__":
    for c in sys.argv[1:] or list(CASES):
        CASES[c]()
