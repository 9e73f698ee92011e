"""CPU-only: the conditional-simulation entry points (carma_simulate_cond_carma / _car1) check their arguments before any
device work and name the path at fault, fail loudly without a GPU, and CarmaSample.makeKalmanFilter('random') is the
reference's random draw from the posterior."""
import ctypes as C

import numpy as np
import pytest

EINVAL, ENODEV = -22, -19


@pytest.fixture(scope="module")
def L():
    import carma_pack_amd._lib as lib
    return lib


def _series(n=6):
    t = np.arange(float(n))
    return t, np.sin(t), 0.1 * np.ones(n)


def _call_carma(L, t, y, e, sig, om, ma, nma, mu, ts, K=None, M=None, p=None):
    om = np.ascontiguousarray(om, dtype=float)
    K = len(sig) if K is None else K
    M = ts.size if M is None else M
    p = om.shape[1] if p is None else p
    out = np.zeros((max(K, 1), max(M, 1)))
    sig, ma = np.ascontiguousarray(sig, dtype=float), np.ascontiguousarray(ma, dtype=float)
    return L.lib.carma_simulate_cond_carma(L.ptr(t), L.ptr(y), L.ptr(e), t.size, p, K, L.ptr(sig), L.ptr(om), L.ptr(ma), nma,
                                           None if mu is None else L.ptr(mu), L.ptr(ts), M, C.c_uint64(1), 0, L.ptr(out),
                                           None, None, None, None, 0)


def _call_car1(L, t, y, e, sig, om, ts, K=None, M=None):
    sig, om = np.ascontiguousarray(sig, dtype=float), np.ascontiguousarray(om, dtype=float)
    K = sig.size if K is None else K
    M = ts.size if M is None else M
    out = np.zeros((max(K, 1), max(M, 1)))
    return L.lib.carma_simulate_cond_car1(L.ptr(t), L.ptr(y), L.ptr(e), t.size, K, L.ptr(sig), L.ptr(om), None, L.ptr(ts), M,
                                          C.c_uint64(1), 0, L.ptr(out), None, None, None, None, 0)


# three good CARMA(3, .) models as [K][p][2] root tables, and one whose complex root has no mate
GOOD = np.array([[[-0.1, -1.0], [-0.1, 1.0], [-0.3, 0.0]]] * 3)
MA = np.array([[1.0, 0.5]] * 3)


def test_einval_before_device_work_names_the_path(L):
    t, y, e = _series()
    ts = np.array([0.5, 7.0])
    sig = np.ones(3)
    # npaths < 1, M < 1
    assert _call_carma(L, t, y, e, sig, GOOD, MA, 2, None, ts, K=0) == EINVAL and "npaths" in L.last_error()
    assert _call_carma(L, t, y, e, sig, GOOD, MA, 2, None, ts, M=0) == EINVAL and "M" in L.last_error()
    assert _call_car1(L, t, y, e, sig, np.ones(3), ts, K=0) == EINVAL and "npaths" in L.last_error()
    assert _call_car1(L, t, y, e, sig, np.ones(3), ts, M=0) == EINVAL
    # nma outside 1..p
    for nma in (0, 4):
        assert _call_carma(L, t, y, e, sig, GOOD, np.ones((3, 4)), nma, None, ts) == EINVAL and "nma" in L.last_error()
    # roots of path 1 not closed under conjugation: the message names path 1
    bad = GOOD.copy()
    bad[1, 1, 1] = 0.7
    assert _call_carma(L, t, y, e, sig, bad, MA, 2, None, ts) == EINVAL
    assert "path 1" in L.last_error() and "conjugate" in L.last_error()
    bad = GOOD.copy()
    bad[2, 0, 0] = -0.2
    assert _call_carma(L, t, y, e, sig, bad, MA, 2, None, ts) == EINVAL and "path 2" in L.last_error()
    # a model that is no process at all: sigsqr / omega not positive
    assert _call_carma(L, t, y, e, np.r_[1.0, 1.0, 0.0], GOOD, MA, 2, None, ts) == EINVAL and "path 2" in L.last_error()
    assert _call_car1(L, t, y, e, sig, np.r_[1.0, -1.0, 1.0], ts) == EINVAL and "path 1" in L.last_error()
    # fewer than 2 distinct data times
    t1 = np.full(6, 3.0)
    assert _call_carma(L, t1, y, e, sig, GOOD, MA, 2, None, ts) == EINVAL and "distinct" in L.last_error()
    assert _call_car1(L, t1, y, e, sig, np.ones(3), ts) == EINVAL and "distinct" in L.last_error()
    # a requested time that is not a number
    assert _call_carma(L, t, y, e, sig, GOOD, MA, 2, None, np.array([0.5, np.nan])) == EINVAL and "tsim[1]" in L.last_error()
    # the Python front end turns these into ValueError
    with pytest.raises(ValueError, match="path 1"):
        bad = GOOD.copy()
        bad[1, 1, 1] = 0.7
        L.simulate_cond_carma(t, y, e, sig, bad[..., 0] + 1j * bad[..., 1], MA, None, ts)
    with pytest.raises(ValueError):
        L.simulate_cond_carma(t, y, e, np.ones(2), GOOD[..., 0] + 1j * GOOD[..., 1], MA, None, ts)   # 2 sigsqr, 3 models


def test_no_cpu_fallback_without_gpu(L):
    if L.lib.carma_device_count() > 0:
        pytest.skip("a GPU is visible")
    t, y, e = _series()
    ts = np.array([0.5, 7.0])
    assert _call_carma(L, t, y, e, np.ones(3), GOOD, MA, 2, None, ts) == ENODEV
    assert _call_car1(L, t, y, e, np.ones(3), np.ones(3), ts) == ENODEV
    with pytest.raises(L.CarmaDeviceError):
        L.simulate_cond_car1(t, y, e, np.ones(3), np.ones(3), None, ts)


def test_merged_times_is_the_grid_of_simulate(L):
    """The grid restated by the Python front end: data first among equal times, positions in the caller's order."""
    t = np.array([3.0, 1.0, 2.0, 2.0])                        # unsorted, one repeated time (dropped)
    ts = np.array([2.5, 0.0, 2.0, 9.0, 2.5])
    grid, dpos, spos = L.merged_times(t, ts)
    assert grid.tolist() == [0.0, 1.0, 2.0, 2.0, 2.5, 2.5, 3.0, 9.0]
    assert dpos.tolist() == [1, 2, 6] and spos.tolist() == [4, 0, 3, 7, 5]


def test_tune_switch_is_known(L):
    L.tune_set("CSIM_CHUNK_PATHS", 3)
    L.tune_set("CSIM_CHUNK_PATHS", None)
    with pytest.raises(ValueError):
        L.tune_set("CSIM_NO_SUCH_SWITCH", 1)


class _Trace(object):
    """A sampler that only holds a trace: what CarmaSample needs on a machine without a GPU."""

    def __init__(self, trace, logpost):
        self._t, self._lp = trace, logpost

    def getSamples(self):
        return self._t

    def GetLogLikes(self):
        return self._lp


def test_make_kalman_filter_random_is_a_posterior_draw(monkeypatch):
    import carma_pack_amd.carma_pack as cp
    rng = np.random.RandomState(0)
    ns, p, q = 40, 3, 1
    trace = np.c_[1.0 + 0.1 * rng.rand(ns), 1.0 + 0.1 * rng.rand(ns), rng.randn(ns), rng.randn(ns, p) - 2.0, rng.randn(ns, q)]
    t = np.arange(8.0)
    # the two derived quantities that come from the device are not under test here
    monkeypatch.setattr(cp.CarmaSample, "_sigma_noise", lambda self: self._samples.__setitem__("sigma", np.arange(1.0, ns + 1.0)))
    sampler = _Trace(trace, -rng.rand(ns))
    sampler.getLogDensityBatch = lambda tr: np.zeros(len(tr))
    sample = cp.CarmaSample(t, np.sin(t), 0.1 * np.ones(8), sampler, q=q)
    sig = np.ravel(sample._samples["sigma"])
    picks = []
    np.random.seed(7)
    for _ in range(25):
        kf, mu = sample.makeKalmanFilter("random")
        i = int(np.flatnonzero(np.isclose(sig ** 2, kf._sigsqr))[0])      # sigma = 1..ns identifies the sample
        assert 0 <= i < ns and mu == float(np.ravel(sample._samples["mu"])[i])
        assert np.array_equal(kf._omega, sample._samples["ar_roots"][i]) and np.array_equal(kf._ma, sample._samples["ma_coefs"][i])
        picks.append(i)
    assert len(set(picks)) > 5                                             # draws, not one fixed sample
    np.random.seed(7)
    again = [int(round(np.sqrt(sample.makeKalmanFilter("random")[0]._sigsqr))) - 1 for _ in range(25)]
    assert again == picks                                                  # reproduces under np.random.seed
    # the point estimates and integer indices are what they were
    assert sample.makeKalmanFilter(4)[0]._sigsqr == 25.0 and sample.makeKalmanFilter(np.int64(4))[1] == trace[4, 2]
    assert sample.makeKalmanFilter("map")[0]._sigsqr == sig[int(np.argmax(sampler._lp))] ** 2
