"""Many series per launch (carma_mseries.hip, its launch plan in carma_mseries_plan.h) against the single-series lane kernel and against a loop over contexts.
One JSON line per case on stdout (and appended to the file MSERIES_PROBE_OUT names, when it is set):
  equal    S = 4096 series x 256 evaluations of CARMA(5,3), n = 270 each (2^20 evaluations)
  ragged   the same with n log-uniform in 50 .. 5000
  car1_S   S = 10^3 and 10^4 series of CAR(1), n = 270, 64 evaluations each
  get_mle  CarmaModelSet.get_mle of 1000 CAR(1) series, split into drawing the starts and the lock-step optimisation
Times are host wall-clock around calls that end in a stream synchronise, median of REPS after a warm-up; every rate includes
the host <-> device copies of the parameter vectors and results, for both sides of a comparison.  The loop over contexts is
timed on LOOP_S series and scaled to S (stated in the line).  Kernel times: run under rocprofv3 --kernel-trace --stats."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import carma_pack_amd as cpa  # noqa: E402
from carma_pack_amd.synth import irregular_series, theta_batch  # noqa: E402

REPS = int(os.environ.get("MSERIES_PROBE_REPS", "5"))
LOOP_S = int(os.environ.get("MSERIES_PROBE_LOOP_S", "512"))
OUT = os.environ.get("MSERIES_PROBE_OUT")


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


def reference_rate(p, q, B):
    """Single-series lane kernel: one n = 270 series, B evaluations in one call."""
    t, y, e = irregular_series(270, seed=1)
    ctx = cpa.Context(t, y, e, p, q)
    th = theta_batch(np.random.default_rng(0), 4096, p, q, t, y)
    th = np.ascontiguousarray(np.tile(th, (B // 4096 + 1, 1))[:B])
    med, lo, hi = timed(lambda: ctx.logdensity(th))
    return ctx.kernel_name(B), med, lo, hi


def case(name, p, q, lengths, per_series, seed, ref=None):
    S = len(lengths)
    series = [irregular_series(int(n), seed=seed + s) for s, n in enumerate(lengths)]
    mc = cpa.MultiContext(series, p, q)
    rng = np.random.default_rng(seed)
    base = [theta_batch(rng, 16, p, q, t, y) for t, y, _ in series]
    th = np.concatenate([np.tile(b, (per_series // 16 + 1, 1))[:per_series] for b in base])
    which = np.repeat(np.arange(S), per_series)
    B = th.shape[0]
    med, lo, hi = timed(lambda: mc.logdensity(th, which))
    steps = float(np.sum(mc.n[which] - 1))
    rec = dict(case=name, p=p, q=q, nseries=S, evals=B, n_min=int(mc.n.min()), n_max=int(mc.n.max()), n_mean=float(mc.n.mean()),
               kernel=mc.kernel_name(), t_s=med, t_min_s=lo, t_max_s=hi, evals_per_s=B / med, eval_steps_per_s=steps / med)
    if ref is not None:
        kname, rmed, _, _ = ref
        rec.update(ref_kernel=kname, ref_t_s=rmed, ref_evals_per_s=B / rmed, ref_eval_steps_per_s=B * 269.0 / rmed,
                   evals_rate_vs_ref=(B / med) / (B / rmed), steps_rate_vs_ref=(steps / med) / (B * 269.0 / rmed))
    # the same work as a loop over single-series contexts (contexts made beforehand), LOOP_S of them, scaled to S
    L = min(LOOP_S, S)
    ctxs = [cpa.Context(*series[s], p, q) for s in range(L)]
    sub = [np.ascontiguousarray(th[which == s]) for s in range(L)]

    def loop():
        for c, x in zip(ctxs, sub):
            c.logdensity(x)
    lmed, _, _ = timed(loop, reps=max(1, REPS // 2))
    rec.update(loop_series_timed=L, loop_t_s=lmed * S / L, speedup_vs_loop=(lmed * S / L) / med,
               loop_kernel=ctxs[0].kernel_name(per_series))
    emit(rec)


def get_mle_case(S=1000, n=200, ntrials=16, seed=3):
    import carmcmc as cm
    series = []
    for s in range(S):
        t, y, e = irregular_series(n, seed=seed + s)
        series.append((t, y, e))
    ms = cm.CarmaModelSet(series, p=1, q=0)
    t0 = time.perf_counter()
    res = ms.get_mle(1, 0, ntrials=ntrials, seed=seed)
    wall = time.perf_counter() - t0
    emit(dict(case="get_mle", p=1, q=0, nseries=S, n=n, ntrials=ntrials, wall_s=wall, starts_s=ms.timing["starts_s"],
              optimise_s=ms.timing["optimise_s"], finite=int(sum(np.isfinite(r.fun) and r.fun < 1e299 for r in res))))


def main():
    assert cpa._lib.lib.carma_device_count() >= 1, "mseries_probe needs a GPU"
    which = sys.argv[1:] or ["equal", "ragged", "car1", "get_mle"]
    if "equal" in which or "ragged" in which:
        ref = reference_rate(5, 3, 1 << 20)
        if "equal" in which:
            case("equal", 5, 3, [270] * 4096, 256, 10000, ref)
        if "ragged" in which:
            n = np.exp(np.random.default_rng(5).uniform(np.log(50), np.log(5000), 4096)).astype(int)
            case("ragged", 5, 3, n, 256, 20000, ref)
    if "car1" in which:
        for S in (1000, 10000):
            case("car1_S%d" % S, 1, 0, [270] * S, 64, 30000, reference_rate(1, 0, S * 64))
    if "get_mle" in which:
        get_mle_case()


if __name__ == "__main__":
    main()
