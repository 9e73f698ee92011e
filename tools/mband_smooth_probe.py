"""The multi-band smoother (carma_bands_smooth) against the route it replaces, README series dealt into three bands.

B = 1, 64, 4096 rows of CARMA(5,3), a random lag per row and band, M requested times of band 1: the wall time of
BandsContext.smooth (host clock around the call, which ends in a device synchronise: copies, both kernels and the chunking
included).  The other column is the only route there was: per row, CarmaBandsModel.merged() on the host and one
smooth_carma call on the merged series (band 0's units, equal shifted times dropped) -- timed over min(B, 64) rows and scaled
to B.  No pass mark: the numbers are the record.

    python tools/mband_smooth_probe.py [--out profiles/mband/smooth_probe_v1.txt] [--M 200] [--reps 5]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import carma_pack_amd as cpa  # noqa: E402
from carma_pack_amd.carma_pack import CarmaBandsModel, mle_to_model  # noqa: E402
from carma_pack_amd.synth import theta_batch  # noqa: E402


def timed(call, reps):
    call()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mband", "smooth_probe_v1.txt"))
    ap.add_argument("--M", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    lib = cpa._lib
    assert lib.lib.carma_device_count() >= 1, "the probe needs a GPU"
    g = np.load(os.path.join(ROOT, "tests", "golden", "carma53_readme.npz"))
    t, y, yerr = g["t"], g["y"], g["yerr"]
    p, q, K, band = 5, 3, 3, 1
    d = 3 + p + q
    bands = [(t[k::K], y[k::K], yerr[k::K]) for k in range(K)]
    model = CarmaBandsModel(bands, p=p, q=q, lag_bounds=[(-10.0, 10.0)] * (K - 1))
    ctx = model.context()
    rng = np.random.default_rng(2)
    base = theta_batch(rng, 4096, p, q, t, y, theta_center=g["theta"][0], frac_post=1.0)
    thx = np.empty((4096, ctx.dx))
    thx[:, :d] = base
    for b in range(1, K):
        thx[:, d + 3 * (b - 1)] = rng.uniform(-10.0, 10.0, 4096)
        thx[:, d + 3 * (b - 1) + 1] = 0.0
        thx[:, d + 3 * (b - 1) + 2] = base[:, 2]
    tout = np.linspace(t[0] - 10.0, t[-1] + 10.0, a.M)
    import torch
    lines = ["mband_smooth_probe: CARMA(%d,%d), README series n = %d in %d bands, M = %d times of band %d, %d timed calls each, %s" % (
        p, q, t.size, K, a.M, band, a.reps, torch.cuda.get_device_name(0))]
    lines.append("scratch %d bytes a row" % (8 * (2 * p + p // 2 + 5) * (t.size + a.M)))

    def merged_loop(rows):
        for x in rows:
            tm, ym, em, _ = model.merged(x)
            sig, roots, ma, mu = mle_to_model(x[:d], p, q)
            lib.smooth_carma(tm, ym, em * np.sqrt(x[1]), [sig], [roots], [ma], [mu], tout - x[d + 3 * (band - 1)], return_singular=True)

    for B in (1, 64, 4096):
        rows = thx[:B]
        dt = timed(lambda: ctx.smooth(rows, band, tout), a.reps)
        nb = min(B, 64)
        dm = timed(lambda: merged_loop(rows[:nb]), 1 if B > 1 else a.reps) * (B / nb)
        lines.append("B = %4d  carma_bands_smooth %10.3f ms  (%.3e row-points/s)   merged() + smooth_carma loop %10.3f ms%s  ratio %.1f" % (
            B, dt * 1e3, B * (t.size + a.M) / dt, dm * 1e3, "" if nb == B else " (from %d rows)" % nb, dm / dt))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
