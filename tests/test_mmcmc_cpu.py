"""CPU-only tests of the multi-series sampler's entry points (carma_mpt_*, CarmaModelSet.run_mcmc, get_mle(starts="set")):
every argument error is reported before any device work, so all of this runs on a machine without a GPU."""
import ctypes as C

import numpy as np
import pytest

from helpers import irregular_series

EINVAL = -22


@pytest.fixture(scope="module")
def cpa():
    import carma_pack_amd
    return carma_pack_amd


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_entry_points_reject_a_null_context(cpa):
    lib = cpa._lib.lib
    x = np.zeros(64)
    w = np.zeros(4, dtype=np.int32)
    wp = w.ctypes.data_as(C.POINTER(C.c_int))
    buf = C.create_string_buffer(64)
    assert lib.carma_mpt_create(None, wp, 1, 10, 1, None, 5, C.c_uint64(1)) == EINVAL
    assert "carma_mpt_create" in cpa._lib.last_error()
    assert lib.carma_mpt_start(None, None) == EINVAL
    assert lib.carma_mpt_set_chains(None, _dp(x), None) == EINVAL
    assert lib.carma_mpt_get_chains(None, _dp(x), _dp(x)) == EINVAL
    assert lib.carma_mpt_get_factor(None, _dp(x)) == EINVAL
    assert lib.carma_mpt_set_factor(None, _dp(x)) == EINVAL
    assert lib.carma_mpt_iterate(None, 1, 1) == EINVAL
    assert lib.carma_mpt_sample(None, 1, 1, _dp(x), _dp(x)) == EINVAL
    assert lib.carma_mpt_stats(None, _dp(x), _dp(x), 0) == EINVAL
    assert lib.carma_mpt_iterations_done(None) == EINVAL
    assert lib.carma_mpt_logdensity(None, _dp(x), _dp(x)) == EINVAL
    assert lib.carma_mpt_kernel_name(None, buf, 64) == EINVAL
    assert lib.carma_mpt_run(None, wp, 1, 10, 1, 5, 5, 1, None, C.c_uint64(1), _dp(x), _dp(x)) == EINVAL


def _set(cpa, p=3, q=1):
    return cpa.CarmaModelSet([irregular_series(n, seed=40 + n) for n in (20, 33, 64)], p, q)


def test_run_mcmc_argument_errors_need_no_device(cpa):
    ms = _set(cpa)
    with pytest.raises(ValueError, match="nsamples"):
        ms.run_mcmc(0)
    with pytest.raises(ValueError, match="ntemperatures"):
        ms.run_mcmc(10, ntemperatures=65)
    with pytest.raises(ValueError, match="ntemperatures"):
        ms.run_mcmc(10, ntemperatures=0)
    with pytest.raises(ValueError, match="nthin"):
        ms.run_mcmc(10, nthin=0)
    with pytest.raises(ValueError, match="nreplicas"):
        ms.run_mcmc(10, nreplicas=0)
    with pytest.raises(ValueError, match="init"):
        ms.run_mcmc(10, init=np.zeros((3, 6)))               # d = 3 + 3 + 1 = 7
    with pytest.raises(ValueError, match="init"):
        ms.run_mcmc(10, init=np.zeros((2, 7)))               # one row per series
    with pytest.raises(ValueError, match="init"):
        _set(cpa, 1, 0).run_mcmc(10, init=np.zeros(4))
    assert ms._mctx == {} and ms.mcmc_samples is None        # no context was ever created


def test_get_mle_rejects_an_unknown_starts_string(cpa):
    ms = _set(cpa)
    with pytest.raises(ValueError, match="starts"):
        ms.get_mle(3, 1, ntrials=4, seed=1, starts="all")
    assert ms._mctx == {}


def test_set_run_sampler_is_what_the_sample_classes_need(cpa):
    from carma_pack_amd import _carmcmc
    for name in ("GetLogLikes", "getSamples", "getAllSamples", "getLogDensityBatch", "SetMLE", "getLogPrior"):
        assert callable(getattr(_carmcmc.SetRunSampler, name))

    class FakeCtx(object):
        p, q, d = 2, 0, 5
        calls = 0

        def logdensity(self, thetas, which, ignore_prior=False):
            FakeCtx.calls += 1
            return np.full(thetas.shape[0], float(which))

    rng = np.random.default_rng(0)
    samples, lps, ll = rng.normal(size=(2, 6, 5)), rng.normal(size=(2, 6)), rng.normal(size=6)
    run = _carmcmc.SetRunSampler(FakeCtx(), 3, samples, lps, ll)
    assert np.array_equal(np.array(run.getSamples()), samples[0]) and np.array_equal(np.array(run.GetLogLikes()), lps[0])
    assert run.getAllSamples()[0] is samples
    assert np.array_equal(run.getLogDensityBatch(samples[0]), np.full(6, 3.0))      # prior bounds on: a launch
    run.SetMLE(True)
    assert run.getLogDensityBatch(samples[0]) is ll and FakeCtx.calls == 1          # the prepared slice, no launch
    assert np.array_equal(run.getLogDensityBatch(samples[1]), np.full(6, 3.0)) and FakeCtx.calls == 2
    s = 1.3
    assert run.getLogPrior([1.0, s, 0.0, 0.0, 0.0]) == pytest.approx(-25.0 / s - 26.0 * np.log(s), rel=1e-15)
