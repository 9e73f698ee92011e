#!/usr/bin/env python3
"""Two builds of the library must pick the same kernels and give the same bits (profiles/r09).  One build per run, chosen by
CARMA_LIB_PATH, so that the outputs of two runs can be compared as files:
  shape_ab.py names             what carma_logdensity_kernel_name, carma_pt_kernel_in_use and carma_pt_row_pipeline answer over the
                                evaluation and ladder counts at which the choice changes, at this device's CU count -> stdout
  shape_ab.py bits OUT.npz      log-densities of a fixed pool of prior-like thetas at p = 5, 3, 7 on the README series in launches of
                                512 ... 4097 evaluations, and the chains of 200 iterations of the row sampler at 16 x 64 from one seed
  shape_ab.py samplers OUT.npz  chains, factors, statistics and 25 samples of the ladder, row, lane and multi-series samplers at
                                16 x 64 after 200 iterations from one seed
  shape_ab.py cmp A.npz B.npz   np.array_equal of every array of two such files
  shape_ab.py calls             wall time of 10^4 back-to-back carma_logdensity_batch_dev calls at B = 16, five times"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
COUNTS = (512, 513, 1024, 1025, 1536, 1537, 3072, 3073, 4096, 4097)


def readme():
    g = np.load(os.path.join(ROOT, "tests", "golden", "carma53_readme.npz"))
    return g["t"], g["y"], g["yerr"]


def names():
    import torch
    import carma_pack_amd as cpa
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    t, y, e = readme()
    k = 100
    series = {"readme": (t, y, e), "close-pair": (np.insert(t, k + 1, t[k] + 0.01), np.insert(y, k + 1, y[k]), np.insert(e, k + 1, e[k])),
              "regular": (np.arange(90.0) * 0.75, y[:90], e[:90]), "n15": (t[:15], y[:15], e[:15])}
    counts = sorted({b for f in (2, 4, 6, 12, 16, 32, 48, 64, 96, 112, 128, 192, 256) for b in (f * cus - 1, f * cus, f * cus + 1)} | {1, 2048, 4096, 8192, 16384})
    print("cus", cus)
    for name, (ts, ys, es) in series.items():
        for p in range(1, 8):
            ctx = cpa.Context(ts, ys, es, p, max(p - 1, 0))
            for B in counts:
                print("name", name, p, B, ctx.kernel_name(B))
    for p, T, n, Rs in ((5, 16, 270, (cus // 4, cus // 4 + 1, cus // 2 + 1, 3 * cus // 4, 3 * cus // 4 + 1, cus, cus + 1)), (5, 10, 270, (1,)),
                        (5, 65, 270, (1,)), (3, 16, 270, (cus // 4, cus)), (7, 16, 270, (cus // 4, cus)), (1, 1, 63, (63, 64, 48 * cus, 64 * cus + 1)),
                        (1, 1, 64, (63, 64, 48 * cus, 48 * cus + 1, 64 * cus, 64 * cus + 1))):
        ctx = cpa.Context(t[:n], y[:n], e[:n], p, 3 if p == 5 else 0)
        for R in Rs:
            for force in (None, "ladder", "row", "lane"):
                os.environ.pop("CARMA_PT_KERNEL", None)
                if force:
                    os.environ["CARMA_PT_KERNEL"] = force
                ctx.pt_create(T, R, adapt_iters=10, seed=1)
                pipe = ""
                if ctx.pt_kernel() == "row" and force is None:
                    ctx.pt_start(None)
                    ctx.pt_iterate(2)
                    pipe = "%s %s" % (ctx.pt_kernel(), cpa.Context.pt_row_pipeline())
                print("sampler", p, T, n, R, force, ctx.pt_kernel(), pipe)
    os.environ.pop("CARMA_PT_KERNEL", None)


def bits(out):
    import carma_pack_amd as cpa
    from helpers import prior_like_theta
    t, y, e = readme()
    res = {}
    for p, q in ((5, 3), (3, 1), (7, 6)):
        rng = np.random.default_rng(900 + p)
        pool = np.array([prior_like_theta(rng, p, q, t, y) for _ in range(4097)])
        ctx = cpa.Context(t, y, e, p, q, max_stdev=10.0 * y.std())
        for B in COUNTS:
            res["ld_p%d_B%d" % (p, B)] = ctx.logdensity(pool[:B])
    ctx = cpa.Context(t, y, e, 5, 3, max_stdev=10.0 * y.std())
    ctx.pt_create(16, 64, adapt_iters=100, seed=11)
    ctx.pt_start(None)
    ctx.pt_iterate(200)
    res["row_kernel"] = np.array([ctx.pt_kernel() + " " + str(cpa.Context.pt_row_pipeline())])
    res["row_theta"], res["row_lp"] = ctx.pt_get_chains()
    np.savez(out, **res)
    print("wrote", out, len(res), "arrays;", res["row_kernel"][0])


def samplers(out):
    """Chains, factors, statistics and samples of the ladder, row, lane and multi-series samplers at 16 x 64 from one seed after 200
    iterations (profiles/r10)."""
    import carma_pack_amd as cpa
    t, y, e = readme()
    ms = 10.0 * y.std()
    res = {}

    def record(name, s):
        s.pt_start(None)
        s.pt_iterate(200)
        res[name + "_theta"], res[name + "_lp"] = s.pt_get_chains()
        res[name + "_factor"] = s.pt_get_factor()
        res[name + "_accept"], res[name + "_swap"] = s.pt_stats()
        res[name + "_samples"], res[name + "_sample_lp"] = s.pt_sample(25, thin=2)

    for kern in ("ladder", "row", "lane"):
        os.environ["CARMA_PT_KERNEL"] = kern
        ctx = cpa.Context(t, y, e, 5, 3, max_stdev=ms)
        ctx.pt_create(16, 64, adapt_iters=100, seed=11)
        res[kern + "_kernel"] = np.array([ctx.pt_kernel()])
        record(kern, ctx)
    os.environ.pop("CARMA_PT_KERNEL", None)
    mc = cpa.MultiContext([(t, y, e), (t[:150], y[:150], e[:150])], 5, 3)
    mc.pt_create([0, 1], 16, 32, adapt_iters=100, seed=11)         # two runs of 32 ladders: 64 ladders of 16
    record("multi", mc)
    np.savez(out, **res)
    print("wrote", out, len(res), "arrays;", " ".join(res[k + "_kernel"][0] for k in ("ladder", "row", "lane")))


def cmp(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files)
    bad = 0
    for k in sorted(A.files):
        same = np.array_equal(A[k], B[k], equal_nan=A[k].dtype.kind == "f")
        bad += not same
        print(k, A[k].shape, "equal" if same else "DIFFERENT", "(%d finite)" % np.isfinite(A[k]).sum() if A[k].dtype.kind == "f" else A[k][0])
    sys.exit(1 if bad else 0)


def calls():
    import torch
    import carma_pack_amd as cpa
    from carma_pack_amd.synth import theta_batch
    g = np.load(os.path.join(ROOT, "tests", "golden", "carma53_readme.npz"))
    t, y, e = readme()
    ctx = cpa.Context(t, y, e, 5, 3, max_stdev=10.0 * y.std())
    th = torch.from_numpy(theta_batch(np.random.default_rng(2), 16, 5, 3, t, y, theta_center=g["theta"][0])).cuda()
    o = torch.empty(16, dtype=torch.float64, device="cuda")
    for _ in range(500):
        ctx.logdensity_dev(th.data_ptr(), 16, o.data_ptr())
    walls = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10000):
            ctx.logdensity_dev(th.data_ptr(), 16, o.data_ptr())
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    print("calls_B16_10000_wall_ms", " ".join("%.2f" % (1e3 * w) for w in walls), "min %.2f" % (1e3 * min(walls)))


if __name__ == "__main__":
    {"names": names, "bits": bits, "samplers": samplers, "cmp": cmp, "calls": calls}[sys.argv[1]](*sys.argv[2:])
