"""The interpolated light curves of many multi-band objects: ONE carma_bandset_smooth call (BandsSetContext.smooth) against the
loop it replaces, one BandsContext.smooth call per (object, band) on a handle per object.  Host wall-clock around calls that end
in a stream synchronise, copies included on both sides, both routes in this process: a warm-up call of each, then the median of
REPS.  One JSON line per case on stdout (and appended to the file MBANDSET_SMOOTH_PROBE_OUT names, when it is set):

  rows1    S objects x K bands x ONE row each  -- what follows CarmaBandsSet.get_mle; every wave of the set call holds one live lane
  rows64   S objects x K bands x 64 rows each  -- full waves

Objects of K = 3 bands of 90 data (N = 270), CARMA(5,3), M times a curve.  The outputs of the two routes are compared for bit
equality.  Expectation to hold the figures against: the kernels' work per row is the same on both sides, since the bodies are
shared; the set's gain is the host side (two launches, one set of copies, one stream sync for all S K curves instead of S K of
each) and, at one row a call, S K waves on the chip at once instead of one."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = int(os.environ.get("MBANDSET_SMOOTH_PROBE_REPS", "7"))
S = int(os.environ.get("MBANDSET_SMOOTH_PROBE_S", "256"))
M = int(os.environ.get("MBANDSET_SMOOTH_PROBE_M", "200"))
OUT = os.environ.get("MBANDSET_SMOOTH_PROBE_OUT")
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


def problem(per):
    """(objects, lag boxes, thx [S][per, dx], times [S][M]): every object its own series, every row its own lags."""
    from carma_pack_amd.synth import irregular_series, theta_batch
    rng = np.random.default_rng(2)
    objs, rows, times = [], [], []
    for s in range(S):
        bands = []
        for b in range(K):
            t, y, e = irregular_series(NB, seed=1000 + K * s + b)
            bands.append((t + 0.7 * b, 1.0 * b + (1.0 + 0.5 * b) * (y - 17.0) + 17.0, e))
        objs.append(bands)
        th = np.tile(theta_batch(rng, min(per, 16), P, Q, bands[0][0], bands[0][1]), (per // 16 + 1, 1))[:per]
        ex = np.column_stack([rng.uniform(-40.0, 40.0, per), np.log(1.5) + 0.1 * rng.standard_normal(per), 1.0 + 0.3 * rng.standard_normal(per),
                              rng.uniform(-40.0, 40.0, per), np.log(2.0) + 0.1 * rng.standard_normal(per), 2.0 + 0.3 * rng.standard_normal(per)])
        rows.append(np.ascontiguousarray(np.hstack([th, ex])))
        lo, hi = min(b[0][0] for b in bands), max(b[0][-1] for b in bands)
        times.append(np.linspace(lo - 10.0, hi + 10.0, M))
    return objs, np.array([(-50.0, 50.0)] * (K - 1)), rows, times


def case(cpa, name, per):
    objs, boxes, rows, times = problem(per)
    ms = [10.0 * o[0][1].std() for o in objs]
    st = cpa.BandsSetContext(objs, P, Q, lag_bounds=boxes, max_stdev=ms)
    ctxs = [cpa.BandsContext(o, P, Q, lag_bounds=boxes, max_stdev=m) for o, m in zip(objs, ms)]
    thx = np.ascontiguousarray(np.concatenate([rows[s] for s in range(S) for _ in range(K)]))
    which = np.repeat(np.arange(S), K * per)
    band = np.tile(np.repeat(np.arange(K), per), S)
    tl = [times[s] for s in which]
    out = {}

    def set_call():
        out["set"] = st.smooth(thx, which, band, tl, return_invalid=True)

    def loop():
        out["loop"] = [c.smooth(rows[s], b, times[s]) for s, c in enumerate(ctxs) for b in range(K)]
    tset, tloop = timed(set_call), timed(loop)
    lm = np.concatenate([m for m, _, _ in out["loop"]])
    lv = np.concatenate([v for _, v, _ in out["loop"]])
    same = np.array_equal(np.array(out["set"][0]), lm, equal_nan=True) and np.array_equal(np.array(out["set"][1]), lv, equal_nan=True)
    B = thx.shape[0]
    emit(cpa, dict(case=name, p=P, q=Q, nbands=K, nobjects=S, N=K * NB, M=M, rows_per_curve=per, rows=B, reps=REPS,
                   invalid=int(np.sum(out["set"][2])), set_t_s=tset[0], set_t_min_s=tset[1], set_t_max_s=tset[2], loop_t_s=tloop[0],
                   loop_t_min_s=tloop[1], loop_t_max_s=tloop[2], set_us_per_row=1e6 * tset[0] / B, loop_us_per_row=1e6 * tloop[0] / B,
                   speedup_vs_loop=tloop[0] / tset[0], same_bits=bool(same)))
    st.close()
    for c in ctxs:
        c.close()


def main():
    import carma_pack_amd as cpa
    assert cpa._lib.lib.carma_device_count() >= 1, "mbandset_smooth_probe needs a GPU"
    case(cpa, "rows1", 1)
    case(cpa, "rows64", 64)


if __name__ == "__main__":
    main()
