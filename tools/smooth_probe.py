"""The one-pass smoother (carma_smooth_* / carma_msmooth) against the per-time calls it is an alternative to (carma_kf_predict,
carma_mpredict), which this work leaves as they were.  One JSON line per case on stdout, and profiles/smooth/README.md (or the
file SMOOTH_PROBE_README names) rewritten with the table:
  shapes   n = 270 with M = 1, 64, 256, 1000, 4000 requested times; n = 3000 with M = 1000; K = 1, 256, 1024 models on the series
  models   CARMA(5,3) (lane groups of 8) and CAR(1) (a lane per model); K models = one model with its time scales spread by +-10 %
  per time K = 1: KalmanFilterp / KalmanFilter1.PredictBatch(times) (series resident in a handle)
           K > 1: MultiContext.predict with K items on the one series, every item at the same times
  smooth   K = 1: .SmoothBatch(times);   K > 1: smooth_carma / smooth_car1 (rows) and band='only' (the K x M arrays stay on the
           device), and MultiContext.smooth with the same items
Times are host wall-clock around calls that return host arrays (each ends in a device synchronise), all copies and allocations
included on both sides; a warm-up call, then the median of REPS.  A case whose per-time side would walk more than
SMOOTH_PROBE_MAX_STEPS recursion steps (K M n) is timed on fewer models and scaled to K, and says so.
Kernel times: run under rocprofv3 --kernel-trace --stats and read k_smooth_* / k_msmooth_* / k_predict_* / k_mpredict_*."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import carma_pack_amd as cpa  # noqa: E402
from carma_pack_amd import _carmcmc as cm  # noqa: E402
from carma_pack_amd.synth import irregular_series  # noqa: E402

REPS = int(os.environ.get("SMOOTH_PROBE_REPS", "5"))
KS = [int(k) for k in os.environ.get("SMOOTH_PROBE_K", "1,256,1024").split(",")]
MAX_STEPS = float(os.environ.get("SMOOTH_PROBE_MAX_STEPS", "3e10"))
README = os.environ.get("SMOOTH_PROBE_README", os.path.join(ROOT, "profiles", "smooth", "README.md"))
SHAPES = [(270, 1), (270, 64), (270, 256), (270, 1000), (270, 4000), (3000, 1000)]

HEAD = """# One-pass smoother: the interpolated light curve and its posterior band (`carma_smooth_carma` / `_car1`, `carma_msmooth`)

What is here:

- `kernel_resources.txt` -- registers, LDS, scratch and occupancy of the kernels (`tools/kernel_resources.sh
  carma_pack_amd/csrc/carma_smooth.hip k_smooth`): no scratch (spill) memory anywhere; `k_smooth_carma<7,8>` 212 VGPRs (2 waves per
  SIMD, as `k_predict_carma`), 3 KiB of LDS per wave for the two group exchanges.

How to measure (one MI355X):

    python tools/smooth_probe.py carma car1
    SMOOTH_PROBE_REPS=3 rocprofv3 --kernel-trace --stats -d prof -o t -- python tools/smooth_probe.py carma

`tools/smooth_probe.py` times the smoother against the per-time calls (`PredictBatch` for one model, `MultiContext.predict` for K
models on the series; neither is touched by the smoother's code) end to end: n = 270 with M = 1, 64, 256, 1000, 4000 requested
times and n = 3000 with M = 1000, K = 1, 256, 1024 models, CARMA(5,3) and CAR(1); a warm-up, then the median of 5 calls, host
wall-clock, every copy and allocation included on both sides.  By step counts the smoother walks 2 (n + M) recursion steps per
model where the per-time route walks M n -- but those M n steps are M (K M) independent lane groups that run side by side, while
a model's smoother is one serial chain: where the two cross depends on how many models share the call.  No speed figure is
asserted anywhere in the test-suite.

"""


def timed(fn, reps=REPS):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def models(p, K):
    """K stable models of order p (p = 5: CARMA(5,3)): one model, its time scales spread by +-10 %."""
    s = np.random.default_rng(5).uniform(0.9, 1.1, K)
    if p == 1:
        return 0.05 * s, None
    roots = np.array([-0.03 - 0.35j, -0.03 + 0.35j, -0.12 - 1.1j, -0.12 + 1.1j, -0.4])
    c = np.poly([-0.6, -1.3, -2.2])
    ma = (c / c[-1])[::-1]
    return roots[None, :] * s[:, None], np.tile(ma, (K, 1))


def case(name, p, rows):
    for n, M in SHAPES:
        t, y, e = irregular_series(n, seed=7)
        y = y - y.mean()
        span = t[-1] - t[0]
        times = np.linspace(t[0] - 0.05 * span, t[-1] + 0.1 * span, M)
        for K in KS:
            roots, ma = models(p, K)
            sig = np.full(K, np.var(y) * (2.0 * 0.05 if p == 1 else 1.0))
            rec = dict(case=name, p=p, n=n, M=M, K=K, reps=REPS)
            Kp = int(max(1, min(K, MAX_STEPS // (float(M) * n))))        # models the per-time side is timed on
            if K == 1:
                tv, yv, ev = cm.vecD(t.tolist()), cm.vecD(y.tolist()), cm.vecD(e.tolist())
                if p == 1:
                    kf = cm.KalmanFilter1(tv, yv, ev, float(sig[0]), float(roots[0]))
                else:
                    kf = cm.KalmanFilterp(tv, yv, ev, float(sig[0]), cm.vecC(roots[0].tolist()), cm.vecD(ma[0].tolist()))
                rec["per_time_s"] = timed(lambda: kf.PredictBatch(times))[0]
                rec["smooth_s"] = timed(lambda: kf.SmoothBatch(times))[0]
            else:
                ctx = cpa.MultiContext([(t, y, e)], p, 3 if p > 1 else 0)
                which = np.zeros(K, dtype=int)
                r_items = -roots if p == 1 else roots
                rec["per_time_s"] = timed(lambda: ctx.predict(which[:Kp], sig[:Kp], r_items[:Kp], None if ma is None else ma[:Kp],
                                                              [times] * Kp))[0] * K / Kp
                rec["per_time_models_timed"] = Kp
                rec["set_smooth_s"] = timed(lambda: ctx.smooth(which, sig, r_items, ma, [times] * K))[0]
                ctx.close()
                if p == 1:
                    rec["smooth_s"] = timed(lambda: cpa.smooth_car1(t, y, e, sig, roots, None, times))[0]
                    rec["band_only_s"] = timed(lambda: cpa.smooth_car1(t, y, e, sig, roots, None, times, band="only"))[0]
                else:
                    rec["smooth_s"] = timed(lambda: cpa.smooth_carma(t, y, e, sig, roots, ma, None, times))[0]
                    rec["band_only_s"] = timed(lambda: cpa.smooth_carma(t, y, e, sig, roots, ma, None, times, band="only"))[0]
            rec["speedup"] = rec["per_time_s"] / rec["smooth_s"]
            rec.update(cpa._lib.build_ids())
            print(json.dumps(rec), flush=True)
            rows.append(rec)


def write_readme(rows):
    out = [HEAD]
    if not rows:
        out.append("No figures are recorded here yet: the probe has not been run on an MI355X.\n")
    else:
        out.append("Measured on one MI355X (median of %d, milliseconds; `per time` scaled from fewer models where marked *):\n\n" % REPS)
        out.append("| model | n | M | K | per time | smooth | band only | set smooth | per time / smooth |\n|---|---|---|---|---|---|---|---|---|\n")
        ms = lambda r, k: "%.3g" % (1e3 * r[k]) if k in r else "--"       # noqa: E731
        for r in rows:
            star = "*" if r.get("per_time_models_timed", r["K"]) < r["K"] else ""
            out.append("| %s | %d | %d | %d | %s%s | %s | %s | %s | %.3g |\n" % (
                "CARMA(5,3)" if r["p"] > 1 else "CAR(1)", r["n"], r["M"], r["K"], ms(r, "per_time_s"), star, ms(r, "smooth_s"),
                ms(r, "band_only_s"), ms(r, "set_smooth_s"), r["speedup"]))
        out.append("\nThe crossing: for each (model, n, K) the smallest measured M at which the smoother is ahead --\n\n")
        seen = {}
        for r in rows:
            key = (r["p"], r["n"], r["K"])
            if r["speedup"] > 1.0 and key not in seen:
                seen[key] = r["M"]
        for r in rows:
            key = (r["p"], r["n"], r["K"])
            if key in seen or (key + ("none",)) in seen:
                continue
            seen[key + ("none",)] = None
        for key in sorted(k for k in seen if len(k) == 3):
            out.append("- %s, n = %d, K = %d: M = %d\n" % ("CARMA(5,3)" if key[0] > 1 else "CAR(1)", key[1], key[2], seen[key]))
        for key in sorted(k for k in seen if len(k) == 4):
            out.append("- %s, n = %d, K = %d: not ahead at any measured M\n" % ("CARMA(5,3)" if key[0] > 1 else "CAR(1)", key[1], key[2]))
    os.makedirs(os.path.dirname(os.path.abspath(README)), exist_ok=True)
    with open(README, "w") as f:
        f.write("".join(out))


def main():
    which = [a for a in sys.argv[1:] if not a.startswith("-")] or ["carma", "car1"]
    rows = []
    if "--readme-only" not in sys.argv:
        assert cpa._lib.lib.carma_device_count() >= 1, "smooth_probe needs a GPU"
        if "carma" in which:
            case("carma", 5, rows)
        if "car1" in which:
            case("car1", 1, rows)
    write_readme(rows)


if __name__ == "__main__":
    main()
