"""The shared front of the handle-based lane samplers (carma_pt_front.h) on the MI355X: carma_mpt_*, carma_bands_pt_* and
carma_bandset_pt_* keep their books -- factor_loaded / chol_stale, the sample buffer's capacity and stride, the iteration count --
in ONE place now.  A sampler that is interrupted between two sampling calls (factors read and written back, chains read and
written back with their log-posteriors) must walk on exactly as an uninterrupted twin of the same seed does."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, T, R, ADAPT = 20261021, 3, 2, 50                       # (the 11 iterations all adapt)


@pytest.fixture(scope="module")
def cpa():
    import carma_pack_amd
    assert carma_pack_amd._lib.lib.carma_device_count() >= 1, "no MI355X visible"
    return carma_pack_amd


def _series(n, seed, level=0.0, amp=1.0, t0=0.0):
    rng = np.random.default_rng(seed)
    t = t0 + np.sort(rng.uniform(0.0, 40.0, n))
    return t, level + amp * np.sin(t / 3.0) + 0.2 * rng.standard_normal(n), np.full(n, 0.2)


def _object(K, seed):
    """K bands of 25, 30, 27 points: one signal, shifted, scaled and offset per band"""
    return [_series((25, 30, 27)[b], seed + b, level=1.0 * b, amp=1.0 + 0.5 * b, t0=0.5 * b) for b in range(K)]


def _create(cpa, kind, p, q, K):
    """(context, create): create() makes the sampler of the test's shape anew, with the chains started"""
    if kind == "mpt":
        ctx = cpa.MultiContext([_series(30, 11), _series(30, 12, level=2.0)], p, q)
        args, kw = ([0, 1], T, R, ADAPT), {}
    elif kind == "bands_pt":
        ctx = cpa.BandsContext(_object(K, 20), p, q, lag_bounds=[(-5.0, 5.0)] * (K - 1))
        args, kw = (T, R, ADAPT), {"band_box": ctx.pt_default_box()}
    else:
        ctx = cpa.BandsSetContext([_object(K, 20), _object(K, 30)], p, q, lag_bounds=[(-5.0, 5.0)] * (K - 1))
        lo, hi = (np.array(v) for v in zip(*[ctx.pt_default_box(s) for s in (0, 1)]))
        args, kw = ([0, 1], T, R, ADAPT), {"band_box": (lo, hi)}

    def create():
        ctx.pt_create(*args, seed=SEED, **kw)
        ctx.pt_start()
    return ctx, create


# p, q = 2, 1 with K = 2 bands: dx = 9, the fused bookkeeping kernels; p, q = 5, 3 with K = 3: dx = 17, the wide ones
@pytest.mark.parametrize("kind,p,q,K", [("mpt", 2, 1, 0), ("bands_pt", 2, 1, 2), ("bandset_pt", 2, 1, 2), ("bands_pt", 5, 3, 3),
                                        ("bandset_pt", 5, 3, 3)])
def test_an_interrupted_sampler_walks_on_as_its_twin(cpa, kind, p, q, K):
    ctx, create = _create(cpa, kind, p, q, K)
    try:
        create()
        a1 = ctx.pt_sample(4, thin=2)
        ctx.pt_set_factor(ctx.pt_get_factor())
        ctx.pt_set_chains(*ctx.pt_get_chains())
        a2 = ctx.pt_sample(3, thin=1)                         # fewer samples than the buffer holds: another stride
        done = ctx.pt_iterations_done()
        end = ctx.pt_get_chains() + (ctx.pt_get_factor(),)
        create()
        b1 = ctx.pt_sample(4, thin=2)
        b2 = ctx.pt_sample(3, thin=1)
        assert done == 11 and ctx.pt_iterations_done() == 11
        lead = ((2,) if kind != "bands_pt" else ()) + (R,)
        assert a1[0].shape == lead + (4, ctx._pt_dim()) and a2[1].shape == lead + (3,)
        for got, want, what in zip(a1 + a2 + end, b1 + b2 + ctx.pt_get_chains() + (ctx.pt_get_factor(),),
                                   ("samples 1", "logposts 1", "samples 2", "logposts 2", "chains", "logpost", "factors")):
            assert np.isfinite(got).all() and np.array_equal(got, want), what
    finally:
        ctx.close()
