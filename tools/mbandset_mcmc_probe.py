"""The sampler over a set of multi-band objects (carma_mband_set_pt.hip, CarmaBandsSet.run_mcmc) against a loop over
CarmaBandsModel.run_mcmc, one object at a time.

  python tools/mbandset_mcmc_probe.py          S objects of K = 3 bands of 90 data (N = 270), CARMA(5,3), T = 10 temperatures, with
                                               R = 1 and R = 6 replicas, ITERS iterations (a third of them burn-in): host wall-clock
                                               around whole run_mcmc calls (copies, the loglik and sigma columns and the sample
                                               objects included on both sides), contexts made beforehand.  The set call: median of
                                               REPS after a warm-up; the loop: ONE pass after a warm-up of its first object.  One
                                               JSON line per R on stdout (appended to the file MBANDSET_MCMC_PROBE_OUT names, when set).
                                               set_pt_run_s is BandsSetContext.pt_run alone, the sampler without the columns.

What the figures are held against.  K1 of the set gives every run waves of its own, so the default ladder (T = 10, R = 1) works
with 10 live lanes of 64 -- accepted on the argument that the filter is a dependent chain over the N data and a wave of 10 live
lanes takes the time of a wave of 64, so that R = 6 should cost the set about what R = 1 does (set_t_s of the two lines), and
that 256 runs are one pass of the chip.  The loop pays a launch of one wave per object, iteration and kernel.  The draws of
the two sides are not the same numbers (a run's Philox keys are those of its ladders in the ensemble): tests/
test_gpu_mbandset_pt.py ties a run to its object's own sampler bit for bit."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = int(os.environ.get("MBANDSET_MCMC_PROBE_REPS", "3"))
S = int(os.environ.get("MBANDSET_MCMC_PROBE_S", "256"))
ITERS = int(os.environ.get("MBANDSET_MCMC_PROBE_ITERS", "300"))
OUT = os.environ.get("MBANDSET_MCMC_PROBE_OUT")
P, Q, K, NB, T = 5, 3, 3, 90, 10


def emit(cpa, rec):
    rec.update(cpa._lib.build_ids())
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "a") as f:
            f.write(line + "\n")


def problem():
    """S objects of K bands of NB data each, every object its own series (the objects of tools/mbandset_probe.py)."""
    from carma_pack_amd.synth import irregular_series
    objs = []
    for s in range(S):
        bands = []
        for b in range(K):
            t, y, e = irregular_series(NB, seed=1000 + K * s + b)
            bands.append((t + 0.7 * b, 1.0 * b + (1.0 + 0.5 * b) * (y - 17.0) + 17.0, e))
        objs.append(bands)
    return objs


def main():
    import carma_pack_amd as cpa
    assert cpa._lib.lib.carma_device_count() >= 1, "mbandset_mcmc_probe needs a GPU"
    bs = cpa.CarmaBandsSet(problem(), p=P, q=Q, lag_bounds=[(-50.0, 50.0)] * (K - 1))
    ctx = bs.context()
    for m in bs.models:
        m.context()
    burn = ITERS // 3
    ns = ITERS - burn
    for R in (1, 6):
        def set_call():
            return bs.run_mcmc(ns, nburnin=burn, ntemperatures=T, nreplicas=R, seed=7)

        def set_sampler():
            lo, hi = (np.array(v) for v in zip(*[ctx.pt_default_box(s) for s in range(S)]))
            return ctx.pt_run(np.arange(S), T, R, ns, burn, 1, seed=7, band_box=(lo, hi))

        def timed(fn):
            fn()
            ts = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t0)
            return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

        tset, tpt = timed(set_call), timed(set_sampler)
        bs.models[0].run_mcmc(ns, nburnin=burn, ntemperatures=T, nreplicas=R, seed=7)
        t0 = time.perf_counter()
        out = [m.run_mcmc(ns, nburnin=burn, ntemperatures=T, nreplicas=R, seed=7) for m in bs.models]
        tloop = time.perf_counter() - t0
        assert all(o._all[0].shape == (R, ns, bs.dx) for o in out)
        emit(cpa, dict(case="run_mcmc", p=P, q=Q, nbands=K, nobjects=S, N=K * NB, ntemps=T, nreplicas=R, iterations=ITERS,
                       kernel=ctx.pt_kernel_name(), live_lanes_per_wave=min(64, R * T), set_t_s=tset[0], set_t_min_s=tset[1],
                       set_t_max_s=tset[2], set_pt_run_s=tpt[0], loop_t_s=tloop, loop_passes=1, speedup_vs_loop=tloop / tset[0],
                       set_us_per_object_iteration=1e6 * tset[0] / (S * ITERS), loop_us_per_object_iteration=1e6 * tloop / (S * ITERS)))


if __name__ == "__main__":
    main()
