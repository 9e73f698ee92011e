"""The two-sided window kernel with two workgroups per CU (odd orders: the FOLDED producers -- the single real root rides in the lane of
a slot's last pair, two passes per chunk, a light wave beside the neighbour's recursion wave).  The folded lane performs the operations
the single root's own lane performed, so every evaluation keeps its bits: a pool of 16 thetas evaluated in a launch of 16 (one
workgroup per CU, the unfolded kernel) and tiled to 1023 and 1024 evaluations (two per CU, with and without an idle row) gives the same
values bit for bit, and those agree with the oracle.  Shapes: the orders that fold and two that do not, series of two chunks per half
and with the split between the halves on a chunk edge, a real-root pair in the folded lane, series with long gaps (re-base in front of
every few chunks: the rotation slot at the end of the second pass; chunks cut short and completed with neutral slots), and phases
beyond the table form's range (the wave-wide slow path with the folded lane in it)."""
import numpy as np
import pytest

import oracle as orc
from helpers import assert_parity, irregular_series, loglik_truth, prior_like_theta

RTOL = 1e-10


@pytest.fixture(scope="module")
def cpa():
    import carma_pack_amd
    assert carma_pack_amd._lib.lib.carma_device_count() >= 1, "no MI355X visible"
    return carma_pack_amd


def _gap_series(n, seed):
    """irregular_series with a gap of many times the series' span in front of every 17th datum and a shorter one in front of every
    7th: far longer than the shortest time scale the prior admits (1 / the smallest step), so windows close all the time"""
    t, y, yerr = irregular_series(n, seed)
    k = np.arange(n)
    t = t + np.cumsum(np.where(k % 17 == 16, 40.0 * (t[-1] - t[0]), 0.0) + np.where(k % 7 == 6, 55.0, 0.0))
    return t, y, yerr


def _pool(rng, p, q, t, y, kind):
    pool = np.array([prior_like_theta(rng, p, q, t, y) for _ in range(16)])
    if kind == "realpair":
        # as test_gpu_parity.test_wave_pipeline_real_pairs: a quadratic factor with positive discriminant -- here the LAST factor, whose
        # lane also takes the single root (p < 6: every factor)
        for f in (range(p // 2) if p < 6 else [p // 2 - 1]):
            r1 = 10.0 ** rng.uniform(-2.0, -0.5, 8) * 3.0 ** f
            r2 = r1 * rng.uniform(3.0, 20.0, 8)
            pool[::2, 3 + 2 * f] = np.log(r1 * r2)
            pool[::2, 4 + 2 * f] = np.log(r1 + r2)
    elif kind == "phase":
        # |Im omega| = 3e5 ... 3e6 rad per time unit, steps of 1 ... 3: |Im omega| dt is beyond CEXP_TAB_MAXPHASE = 98304
        pool[1::4, 3] = 2.0 * np.log(3e5 * 10.0 ** rng.uniform(0.0, 1.0, 4))
    return pool


CASES = [
    # name, p, q, series, n, thetas
    ("order53", 5, 3, "irregular", 150, "prior"),
    ("order50", 5, 0, "irregular", 150, "prior"),
    ("order76", 7, 6, "irregular", 150, "prior"),
    ("order31", 3, 1, "irregular", 150, "prior"),
    ("order63-untouched", 6, 3, "irregular", 150, "prior"),
    ("order42-untouched", 4, 2, "irregular", 150, "prior"),
    ("n40-53", 5, 3, "irregular", 40, "prior"),
    ("n23-53", 5, 3, "irregular", 23, "prior"),
    ("n24-53", 5, 3, "irregular", 24, "prior"),
    ("n40-76", 7, 6, "irregular", 40, "prior"),
    ("n23-31", 3, 1, "irregular", 23, "prior"),
    ("n24-76", 7, 6, "irregular", 24, "prior"),
    ("realpair53", 5, 3, "irregular", 150, "realpair"),
    ("realpair76", 7, 6, "irregular", 150, "realpair"),
    ("realpair31", 3, 1, "irregular", 150, "realpair"),
    ("gaps53", 5, 3, "gaps", 150, "prior"),
    ("gaps76", 7, 6, "gaps", 150, "prior"),
    ("gaps31", 3, 1, "gaps", 150, "prior"),
    ("phase53", 5, 3, "irregular", 150, "phase"),
    ("phase76", 7, 6, "irregular", 150, "phase"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,p,q,series,n,kind", CASES, ids=[c[0] for c in CASES])
def test_w2_two_workgroups_per_cu_keep_bits(cpa, name, p, q, series, n, kind):
    seed = 800 + n + 10 * p + q
    t, y, yerr = _gap_series(n, seed) if series == "gaps" else irregular_series(n, seed)
    pool = _pool(np.random.default_rng(8000 + seed), p, q, t, y, kind)
    ign = kind != "prior"            # (real pairs and huge frequencies lie outside the prior's bounds)
    ctx = cpa.Context(t, y, yerr, p, q)
    try:
        if ctx.kernel_name(1024) != "k_logdens_carma_w2<%d>" % p:
            cpa._lib.tune_set("WIN_ROWS", 256)       # (an override lifts the series criterion: the gaps fail it)
        for B in (16, 1023, 1024):
            assert ctx.kernel_name(B) == "k_logdens_carma_w2<%d>" % p, (B, ctx.kernel_name(B))
        first = ctx.logdensity(pool, ignore_prior=ign)
        for B in (1023, 1024):
            idx = np.arange(B) % pool.shape[0]
            got = ctx.logdensity(pool[idx], ignore_prior=ign)
            same = (got == first[idx]) | (np.isnan(got) & np.isnan(first[idx]))
            print("%s B=%d: %d of %d differ from the launch of 16" % (name, B, int((~same).sum()), B))
            assert np.array_equal(got, first[idx], equal_nan=True), (name, B, np.flatnonzero(~same)[:8])
        want = orc.OracleModel(t, y, yerr, p, q, max_stdev=ctx.prior()[0]).logdensity_batch(pool, ignore_prior=ign)
        print("%s: %d of 16 finite" % (name, int(np.isfinite(want).sum())))
        assert_parity(first, want, RTOL, "w2 fold %s" % name, arbiter=lambda i: loglik_truth(t, y, yerr, pool[i], p, q)[0])
        if kind != "phase":          # (the huge frequencies are far outside the prior and may well overflow)
            assert np.isfinite(first).sum() >= 8
    finally:
        cpa._lib.tune_reset()
