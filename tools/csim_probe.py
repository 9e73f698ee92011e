"""The posterior-predictive path ensemble in one call (CarmaSample.simulate_paths -> carma_simulate_cond_*) against the loop it
replaces.  One JSON line per case on stdout (and appended to the file CSIM_PROBE_OUT names, when it is set):
  carma   CARMA(5,3), n = 270, M = 500 requested times, K in {16, 256, 4096} paths, a posterior sample each
  car1    CAR(1), likewise
Both sides produce K conditional paths at the same times, path j under posterior sample idx[j]:
  ensemble   sample.simulate_paths(times, K, 'random', seed)                       two launches for all paths
  loop       for j in range(K): sample.simulate(times, bestfit=int(idx[j]))        KalmanFilterp.Simulate per path: two launches,
             two uploads of the series and the allocations of both, per path
Times are host wall-clock around calls that end in a device synchronise, median of REPS after a warm-up, all copies included on
both sides.  The loop is timed on min(K, LOOP_K) paths and scaled to K (stated in the line).  The posterior is a short run of
the sampler on a synthetic series (its quality does not matter here: any set of valid models costs the same).
Kernel times: run under rocprofv3 --kernel-trace --stats with CSIM_PROBE_LOOP_K=0 (no loop) and read k_csim_paths_* /
k_csim_predict_* from the statistics."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import carma_pack_amd as cpa  # noqa: E402
from carma_pack_amd.carma_pack import CarmaModel  # noqa: E402
from carma_pack_amd.synth import irregular_series  # noqa: E402

REPS = int(os.environ.get("CSIM_PROBE_REPS", "5"))
LOOP_K = int(os.environ.get("CSIM_PROBE_LOOP_K", "256"))
KS = [int(k) for k in os.environ.get("CSIM_PROBE_K", "16,256,4096").split(",")]
OUT = os.environ.get("CSIM_PROBE_OUT")
N, M = 270, 500


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


def case(name, p, q):
    t, y, e = irregular_series(N, seed=7)
    sample = CarmaModel(t, y, e, p=p, q=q).run_mcmc(512, nburnin=256, seed=1)
    span = t[-1] - t[0]
    times = np.linspace(t[0] - 0.05 * span, t[-1] + 0.2 * span, M)
    for K in KS:
        e_med, e_lo, e_hi = timed(lambda: sample.simulate_paths(times, K, "random", seed=3))
        rec = dict(case=name, p=p, q=q, n=N, M=M, K=K, reps=REPS, ensemble_s=e_med, ensemble_min_s=e_lo, ensemble_max_s=e_hi,
                   paths_per_s=K / e_med)
        L = min(LOOP_K, K)
        if L > 0:
            idx = np.random.RandomState(3).randint(0, 512, size=K)

            def loop():
                for j in range(L):
                    sample.simulate(times, bestfit=int(idx[j]))
            l_med, l_lo, l_hi = timed(loop, reps=max(1, REPS // 2))
            rec.update(loop_paths_timed=L, loop_s=l_med * K / L, loop_min_s=l_lo * K / L, loop_max_s=l_hi * K / L,
                       speedup_vs_loop=(l_med * K / L) / e_med)
        emit(rec)


def main():
    assert cpa._lib.lib.carma_device_count() >= 1, "csim_probe needs a GPU"
    which = sys.argv[1:] or ["carma", "car1"]
    if "carma" in which:
        case("carma", 5, 3)
    if "car1" in which:
        case("car1", 1, 0)


if __name__ == "__main__":
    main()
