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


# The three handle-based lane samplers share one front (carma_pt_front.h): every entry point of each returns EINVAL on a null
# handle, and every one that sets a message has ITS OWN name at the start of last_error().
@pytest.mark.parametrize("prefix", ["carma_mpt", "carma_bands_pt", "carma_bandset_pt"])
def test_entry_points_reject_a_null_context(cpa, prefix):
    lib = cpa._lib.lib
    x = np.zeros(64)
    w = np.zeros(4, dtype=np.int32)
    wp = w.ctypes.data_as(C.POINTER(C.c_int))
    buf = C.create_string_buffer(64)
    seed = C.c_uint64(1)
    fn = lambda name: getattr(lib, prefix + "_" + name)

    # (consecutive calls below expect different names, so a message left by the call before does not pass)
    def rejected(name, *args, named=None):
        assert fn(name)(None, *args) == EINVAL, name
        if named is not None:
            assert cpa._lib.last_error().startswith(prefix + "_" + named + ":"), (name, cpa._lib.last_error())

    create = {"carma_mpt": (wp, 1, 10, 1, None, 5, seed),
              "carma_bands_pt": (10, 1, None, 5, seed, None, None),
              "carma_bandset_pt": (wp, 1, 10, 1, None, 5, seed, None, None)}[prefix]
    run = {"carma_mpt": (wp, 1, 10, 1, 5, 5, 1, None, seed, _dp(x), _dp(x)),
           "carma_bands_pt": (10, 1, 5, 5, 1, None, seed, None, None, _dp(x), _dp(x)),
           "carma_bandset_pt": (wp, 1, 10, 1, 5, 5, 1, None, seed, None, None, _dp(x), _dp(x))}[prefix]
    rejected("create", *create, named="create")
    rejected("start", None, named="start")
    rejected("set_chains", _dp(x), None, named="set_chains")
    rejected("get_chains", _dp(x), _dp(x), named="get_chains")
    rejected("get_factor", _dp(x), named="get_factor")
    rejected("set_factor", _dp(x), named="set_factor")
    rejected("iterate", 1, 1, named="iterate")
    rejected("sample", 1, 1, _dp(x), _dp(x), named="sample")
    rejected("stats", _dp(x), _dp(x), 0, named="stats")
    rejected("iterations_done")
    rejected("logdensity", _dp(x), _dp(x), named="logdensity")
    rejected("kernel_name", buf, 64)
    rejected("run", *run, named="create")                    # (run's first step is create, which words the refusal)
    if prefix == "carma_bands_pt":
        rejected("default_box", _dp(x), _dp(x), named="default_box")
    if prefix == "carma_bandset_pt":
        rejected("default_box", 0, _dp(x), _dp(x), named="default_box")


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
