"""The two-sided window kernel's prologue copies theta, the math tables and the first 512 records of the series into LDS in one
pass, and the rest of a longer series behind it.  Series lengths either side of 256 and 512 records, at batch sizes of one to three
workgroups per CU and with idle rows: every evaluation's value is the same bits whatever its position in the batch and the batch
size, and agrees with the one-sided window pipeline and with the oracle."""
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


@pytest.mark.gpu
@pytest.mark.parametrize("n", [40, 255, 256, 257, 511, 512, 513, 1100])
@pytest.mark.parametrize("p,q", [(2, 0), (5, 3), (7, 6)])
def test_w2_series_lengths_and_batch_sizes(cpa, n, p, q):
    t, y, yerr = irregular_series(n, seed=500 + n + p)
    rng = np.random.default_rng(7000 + n + 10 * p + q)
    pool = np.array([prior_like_theta(rng, p, q, t, y) for _ in range(16)])
    ctx = cpa.Context(t, y, yerr, p, q)
    try:
        first = None
        for B in (1, 3, 512, 513, 1024):
            assert ctx.kernel_name(B) == "k_logdens_carma_w2<%d>" % p, (B, ctx.kernel_name(B))
            th = pool[np.arange(B) % pool.shape[0]]
            got = ctx.logdensity(th)
            k = min(B, pool.shape[0])
            if first is None:
                first = ctx.logdensity(pool)
            # every copy of a theta, wherever it sits in the batch, has the value it has alone in a launch of 16
            assert np.array_equal(got, first[np.arange(B) % pool.shape[0]], equal_nan=True), (n, B)
            assert np.array_equal(got[:k], first[:k], equal_nan=True)
        want = orc.OracleModel(t, y, yerr, p, q, max_stdev=ctx.prior()[0]).logdensity_batch(pool)
        # (prior-like theta: where the roots cluster the oracle's own arithmetic is off, and the exact value arbitrates)
        arb = lambda i: loglik_truth(t, y, yerr, pool[i], p, q)[0]   # noqa: E731
        assert_parity(first, want, RTOL, "two-sided n=%d p=%d q=%d" % (n, p, q), arbiter=arb)
        cpa._lib.tune_set("WIN2_EVALS", 0)
        assert ctx.kernel_name(16) == "k_logdens_carma_w<%d>" % p
        one_sided = ctx.logdensity(pool)
        assert np.array_equal(np.isfinite(one_sided), np.isfinite(first))
        assert_parity(one_sided, want, RTOL, "one-sided n=%d p=%d q=%d" % (n, p, q), arbiter=arb)
    finally:
        cpa._lib.tune_reset()
