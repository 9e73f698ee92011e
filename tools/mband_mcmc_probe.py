"""The sampler of a multi-band fit (carma_bands_pt_*): time per iteration, split into K1 and bookkeeping.

README series (n = 270) dealt into K bands: dx = 9 (CARMA(2,1), K = 2), 17 ((5,3), K = 3) and 37 ((7,6), K = 8), ensembles from
10 x 1 to 16 x 4096 chains.  Per size: the wall time of an iteration of BandsContext.pt_iterate (frozen factor: past the burn-in;
and adapting: inside it), and the time of K1's work alone -- the batch kernel k_logdens_carma_mband on as many device-resident
evaluations (the body of k_logdens_carma_mband_chains, without the box test), between two events.  Bookkeeping = iteration - K1:
the propose and finish kernels (templated up to dx = 16, the wide ones beyond), their launches and the chunk's two conversions.
Then the wide kernels against the templated ones on a single-series lane sampler at d = 16 (CARMA(7,6)), "PT_RAM_WIDE_MIN" moved.
The claim under test: the bookkeeping is a minor share of an iteration at N >= 100 data.  No pass mark: the numbers are the record.

    python tools/mband_mcmc_probe.py [--out profiles/mband/mcmc_probe_v1.txt] [--iters 60] [--max-chains 65536]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import carma_pack_amd as cpa  # noqa: E402

SIZES = [(10, 1), (10, 64), (16, 256), (16, 1024), (16, 4096)]


def per_iter(ctx, iters):
    ctx.pt_iterate(5)
    t0 = time.perf_counter()
    ctx.pt_iterate(iters)
    return (time.perf_counter() - t0) / iters


def k1_alone(ctx, theta, reps):
    import torch
    dev = torch.device("cuda")
    d_th = torch.from_numpy(np.ascontiguousarray(theta)).to(dev)
    out = torch.empty(theta.shape[0], dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    ctx.logdensity_dev(d_th.data_ptr(), theta.shape[0], out.data_ptr(), ignore_prior=False, stream=st)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ctx.logdensity_dev(d_th.data_ptr(), theta.shape[0], out.data_ptr(), ignore_prior=False, stream=st)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mband", "mcmc_probe_v1.txt"))
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--max-chains", type=int, default=65536)
    a = ap.parse_args()
    lib = cpa._lib
    assert lib.lib.carma_device_count() >= 1, "the probe needs a GPU"
    import torch
    g = np.load(os.path.join(ROOT, "tests", "golden", "carma53_readme.npz"))
    t, y, yerr = g["t"], g["y"], g["yerr"]
    lines = ["mband_mcmc_probe: README series n = %d dealt into K bands, %d timed iterations per entry, %s" % (
        t.size, a.iters, torch.cuda.get_device_name(0))]
    lines.append("per iteration, us: frozen = past the burn-in, adapting = inside it; K1 = k_logdens_carma_mband on as many evaluations; "
                 "book = frozen - K1")
    for p, q, K in ((2, 1, 2), (5, 3, 3), (7, 6, 8)):
        bands = [(t[k::K], y[k::K], yerr[k::K]) for k in range(K)]
        model = cpa.CarmaBandsModel(bands, p=p, q=q, lag_bounds=[(-5.0, 5.0)] * (K - 1))
        ctx = model.context()
        box = ctx.pt_default_box()
        for T, R in SIZES:
            if T * R > a.max_chains:
                continue
            ctx.pt_create(T, R, 0, seed=1, band_box=box)
            ctx.pt_start()
            frozen = per_iter(ctx, a.iters)
            th, _ = ctx.pt_get_chains()
            k1 = k1_alone(ctx, th.reshape(-1, ctx.dx), max(5, a.iters // 4))
            ctx.pt_create(T, R, 10 ** 9, seed=1, band_box=box)
            ctx.pt_start()
            adapting = per_iter(ctx, a.iters)
            lines.append("dx = %2d (p,q,K = %d,%d,%d)  %2d x %4d = %5d chains  frozen %8.1f  adapting %8.1f  K1 %8.1f  book %8.1f (%4.1f %% of frozen, "
                         "%4.1f %% of adapting)" % (ctx.dx, p, q, K, T, R, T * R, frozen * 1e6, adapting * 1e6, k1 * 1e6, (frozen - k1) * 1e6,
                                                  100.0 * (frozen - k1) / frozen, 100.0 * (adapting - k1) / adapting))
            print(lines[-1], flush=True)
        ctx.close()
    # the wide kernels against the templated ones, single-series lane sampler at d = 16
    old = os.environ.get("CARMA_PT_KERNEL")
    os.environ["CARMA_PT_KERNEL"] = "lane"
    try:
        ctx = cpa.Context(t, y, yerr, 7, 6)
        for T, R in ((16, 256), (16, 1024), (16, 4096)):
            if T * R > a.max_chains:
                continue
            row = []
            for wide_min in (None, 4):
                lib.tune_set("PT_RAM_WIDE_MIN", wide_min)
                for adapt in (0, 10 ** 9):
                    ctx.pt_create(T, R, adapt, seed=1)
                    ctx.pt_start()
                    row.append(per_iter(ctx, a.iters) * 1e6)
            lines.append("d = 16, single series n = %d, %2d x %4d chains: templated (split) frozen %8.1f adapting %8.1f   wide frozen %8.1f "
                         "adapting %8.1f" % (t.size, T, R, row[0], row[1], row[2], row[3]))
            print(lines[-1], flush=True)
        ctx.close()
    finally:
        lib.tune_set("PT_RAM_WIDE_MIN", None)
        if old is None:
            del os.environ["CARMA_PT_KERNEL"]
        else:
            os.environ["CARMA_PT_KERNEL"] = old
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
