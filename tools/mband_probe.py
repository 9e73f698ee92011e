"""The multi-band kernel (k_logdens_carma_mband) against the single-series lane kernel, README series, B = 2^16.

K = 1: the same series and parameter vectors through carma_bands_logdensity_batch_dev and through carma_logdensity_batch_dev forced
to the lane kernel (CARMA_TUNE_LANE_MIN=0, set below before the library reads it): the ratio is what the merge costs -- per-lane
record loads and a transition factor per lane and step where the lane kernel has scalar loads (and a skip for repeated steps).
K = 2, 3, 6: the same data dealt round-robin into K bands (the same N steps), a random lag per lane, so that the lanes of a wave
walk different merge orders.  No pass mark: the ratios are the record.

    python tools/mband_probe.py [--out profiles/mband/probe_v1.txt] [--logB 16] [--reps 10]
"""
import argparse
import os
import sys
import time

os.environ.setdefault("CARMA_TUNE_LANE_MIN", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import carma_pack_amd as cpa  # noqa: E402
from carma_pack_amd.synth import theta_batch  # noqa: E402


def timed(call, reps):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mband", "probe_v1.txt"))
    ap.add_argument("--logB", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    assert cpa._lib.lib.carma_device_count() >= 1, "the probe needs a GPU"
    g = np.load(os.path.join(ROOT, "tests", "golden", "carma53_readme.npz"))
    t, y, yerr = g["t"], g["y"], g["yerr"]
    p, q, B = 5, 3, 1 << a.logB
    d = 3 + p + q
    ms = 10.0 * np.sqrt(np.mean(y * y) - np.mean(y) ** 2)
    rng = np.random.default_rng(2)
    base = theta_batch(rng, 4096, p, q, t, y, theta_center=g["theta"][0], frac_post=1.0)
    th = np.tile(base, (B // 4096 + 1, 1))[:B].copy()
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream
    out = torch.empty(B, dtype=torch.float64, device=dev)
    lines = ["mband_probe: CARMA(%d,%d), README series n = %d, B = %d, %d timed launches each, %s" % (
        p, q, t.size, B, a.reps, torch.cuda.get_device_name(0))]

    one = cpa.Context(t, y, yerr, p, q, max_stdev=ms)
    d_th = torch.from_numpy(th).to(dev)
    t_lane = timed(lambda: one.logdensity_dev(d_th.data_ptr(), B, out.data_ptr(), ignore_prior=True, stream=st), a.reps)
    want = out.cpu().numpy()
    lines.append("single series  %-28s %10.1f us/launch  %.3e evaluation-steps/s" % (one.kernel_name(B), t_lane * 1e6, B * t.size / t_lane))
    for K in (1, 2, 3, 6):
        bands = [(t[k::K], y[k::K], yerr[k::K]) for k in range(K)]
        ctx = cpa.BandsContext(bands, p, q, lag_bounds=[(-10.0, 10.0)] * (K - 1), max_stdev=ms)
        thx = np.empty((B, ctx.dx))
        thx[:, :d] = th
        for b in range(1, K):
            thx[:, d + 3 * (b - 1)] = rng.uniform(-10.0, 10.0, B)
            thx[:, d + 3 * (b - 1) + 1] = 0.0
            thx[:, d + 3 * (b - 1) + 2] = th[:, 2]
        d_thx = torch.from_numpy(thx).to(dev)
        dt = timed(lambda: ctx.logdensity_dev(d_thx.data_ptr(), B, out.data_ptr(), ignore_prior=True, stream=st), a.reps)
        note = ""
        if K == 1:
            got = out.cpu().numpy()
            fin = np.isfinite(want)
            note = "  max rel difference from the single-series kernel %.1e" % np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin]))
        lines.append("K = %d bands    %-28s %10.1f us/launch  %.3e evaluation-steps/s  %.2f x the single-series time%s" % (
            K, "k_logdens_carma_mband<%d>" % p, dt * 1e6, B * t.size / dt, dt / t_lane, note))
        ctx.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
