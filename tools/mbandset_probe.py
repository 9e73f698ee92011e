"""Many multi-band objects per launch (carma_mband_set.hip) against a loop over single-object handles (BandsContext), for
log-densities and for lag_profile.  Host call time and kernel time are measured separately:

  python tools/mbandset_probe.py host          host wall-clock around calls that end in a stream synchronise, median of REPS after
                                               a warm-up, copies included on both sides; one JSON line per case on stdout (and
                                               appended to the file MBANDSET_PROBE_OUT names, when it is set):
      logdens      S objects of K = 3 bands of 90 data (N = 270), CARMA(5,3), PER evaluations each: one set call against S calls
      lag_profile  S_FIT objects of 2 x 60 data, CARMA(2,1): CarmaBandsSet.lag_profile against CarmaBandsModel.lag_profile each
  python tools/mbandset_probe.py kernels       the log-density calls of `logdens` alone, both sides once after a warm-up: run it under
                                               rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python ... kernels
                                               (a run of its own: tracing slows the host)
  python tools/mbandset_probe.py summarise DIR  the k_logdens_carma_mband* rows of DIR's kernel_stats.csv as time per evaluation

Expectation to hold the figures against: at equal N and full waves the kernel's time per evaluation equals
k_logdens_carma_mband's, since the body is shared; the set's gain is the host side (one launch, one pair of copies, one stream
sync per step instead of S)."""
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = int(os.environ.get("MBANDSET_PROBE_REPS", "5"))
S = int(os.environ.get("MBANDSET_PROBE_S", "256"))
PER = int(os.environ.get("MBANDSET_PROBE_PER", "256"))
S_FIT = int(os.environ.get("MBANDSET_PROBE_S_FIT", "16"))
OUT = os.environ.get("MBANDSET_PROBE_OUT")
P, Q, K, NB = 5, 3, 3, 90


def timed(fn, reps=REPS):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def emit(cpa, rec):
    rec.update(cpa._lib.build_ids())
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "a") as f:
            f.write(line + "\n")


def logdens_problem(cpa):
    """(objects, lag boxes [K - 1, 2], thx [S PER, dx], which): every object its own series, every lane its own lags."""
    from carma_pack_amd.synth import irregular_series, theta_batch
    rng = np.random.default_rng(1)
    objs, rows = [], []
    for s in range(S):
        bands = []
        for b in range(K):
            t, y, e = irregular_series(NB, seed=1000 + K * s + b)
            bands.append((t + 0.7 * b, 1.0 * b + (1.0 + 0.5 * b) * (y - 17.0) + 17.0, e))
        objs.append(bands)
        th = theta_batch(rng, 16, P, Q, bands[0][0], bands[0][1])
        th = np.tile(th, (PER // 16 + 1, 1))[:PER]
        ex = np.column_stack([rng.uniform(-40.0, 40.0, PER), np.log(1.5) + 0.1 * rng.standard_normal(PER), 1.0 + 0.3 * rng.standard_normal(PER),
                              rng.uniform(-40.0, 40.0, PER), np.log(2.0) + 0.1 * rng.standard_normal(PER), 2.0 + 0.3 * rng.standard_normal(PER)])
        rows.append(np.hstack([th, ex]))
    return objs, np.array([(-50.0, 50.0)] * (K - 1)), np.ascontiguousarray(np.concatenate(rows)), np.repeat(np.arange(S), PER)


def logdens_sides(cpa):
    objs, boxes, thx, which = logdens_problem(cpa)
    ms = [10.0 * o[0][1].std() for o in objs]
    st = cpa.BandsSetContext(objs, P, Q, lag_bounds=boxes, max_stdev=ms)
    ctxs = [cpa.BandsContext(o, P, Q, lag_bounds=boxes, max_stdev=m) for o, m in zip(objs, ms)]
    sub = [np.ascontiguousarray(thx[which == s]) for s in range(S)]
    out = {}

    def set_call():
        out["set"] = st.logdensity(thx, which, ignore_prior=True)

    def loop():
        out["loop"] = np.concatenate([c.logdensity(x, ignore_prior=True) for c, x in zip(ctxs, sub)])
    return st, set_call, loop, out, thx.shape[0]


def host(cpa):
    st, set_call, loop, out, B = logdens_sides(cpa)
    tset, tloop = timed(set_call), timed(loop)
    assert np.array_equal(out["set"], out["loop"]), "the set and the loop disagree"
    emit(cpa, dict(case="logdens", p=P, q=Q, nbands=K, nobjects=S, N=K * NB, evals=B, kernel=st.kernel_name(), set_t_s=tset[0],
                   set_t_min_s=tset[1], set_t_max_s=tset[2], loop_t_s=tloop[0], loop_t_min_s=tloop[1], loop_t_max_s=tloop[2],
                   set_us_per_eval=1e6 * tset[0] / B, loop_us_per_eval=1e6 * tloop[0] / B, speedup_vs_loop=tloop[0] / tset[0]))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mband_ref as R
    objs = [R.recovery_problem(100 + s)[0] for s in range(S_FIT)]
    bs = cpa.CarmaBandsSet(objs, p=2, q=1, lag_bounds=[(-1.0, 9.0)])
    lags, res = R.RECOVERY_LAGS, {}

    def set_fit():
        res["set"] = bs.lag_profile(lags, ntrials=4, seed=11)
        res["timing"] = dict(bs.timing)

    def loop_fit():
        res["loop"] = [m.lag_profile(lags, ntrials=4, seed=11) for m in bs.models]
    reps = max(1, REPS // 2)
    tset, tloop = timed(set_fit, reps), timed(loop_fit, reps)
    same = all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(res["set"], res["loop"]))
    emit(cpa, dict(case="lag_profile", p=2, q=1, nbands=2, nobjects=S_FIT, N=120, lags=int(lags.size), ntrials=4, set_t_s=tset[0],
                   set_t_min_s=tset[1], set_t_max_s=tset[2], set_starts_s=res["timing"]["starts_s"],
                   set_optimise_s=res["timing"]["optimise_s"], loop_t_s=tloop[0], loop_t_min_s=tloop[1], loop_t_max_s=tloop[2],
                   speedup_vs_loop=tloop[0] / tset[0], same_bits=bool(same)))


def kernels(cpa):
    _, set_call, loop, _, B = logdens_sides(cpa)
    for fn in (set_call, loop, set_call, loop):               # a warm-up of each, then the calls the trace is read for
        fn()
    print("kernels: %d evaluations on each side, twice" % B)


def summarise(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit("no kernel_stats.csv under %s" % d)
    B = S * PER
    for row in csv.DictReader(open(files[0])):
        if "k_logdens_carma_mband" in row["Name"]:
            calls, total = int(row["Calls"]), float(row["TotalDurationNs"])
            # the set: 2 launches of B evaluations; the loop: 2 S launches of PER
            print(json.dumps(dict(kernel=row["Name"], calls=calls, total_us=total / 1e3, mean_us=total / 1e3 / calls,
                                  ns_per_eval=total / (2.0 * B))))


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "host"
    if mode == "summarise":
        return summarise(sys.argv[2])
    import carma_pack_amd as cpa
    assert cpa._lib.lib.carma_device_count() >= 1, "mbandset_probe needs a GPU"
    {"host": host, "kernels": kernels}[mode](cpa)


if __name__ == "__main__":
    main()
