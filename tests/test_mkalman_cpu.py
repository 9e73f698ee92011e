"""CPU-only: the host side of the set-wide filter and predict (carma_mkfilter / carma_mpredict, MultiContext.kfilter / predict,
CarmaModelSet.predict / assess_fit) -- the conversion of an MLE vector into the filter's model, the grouping of a set by order,
the shapes predict accepts, and the argument errors that are raised before any library or device call."""
import ctypes as C
import types

import numpy as np
import pytest

import carma_pack_amd as cpa
import oracle as orc
from carma_pack_amd import carma_pack as cp
from helpers import irregular_series, prior_like_theta

L = cpa._lib.lib
EINVAL = -22


@pytest.mark.parametrize("p,q", [(1, 0), (2, 0), (2, 1), (3, 2), (4, 0), (5, 3), (6, 5), (7, 6)])
def test_mle_to_model_is_add_mle_and_the_oracle(p, q):
    """mle_to_model(x, p, q) gives the values CarmaSample.add_mle stores (var / carma_variance(1, roots, ma) = sigma^2, the
    roots, the MA coefficients, mu), and they are the reference's ar_roots / ma_coefs / variance (oracle) to rounding."""
    rng = np.random.default_rng(10 * p + q)
    t, y, _ = irregular_series(60, 3)
    for _ in range(5):
        if p == 1:
            x = np.array([rng.uniform(0.2, 2.0), rng.uniform(0.7, 1.4), rng.normal(), rng.uniform(-4.0, 1.0)])
        else:
            x = prior_like_theta(rng, p, q, t, y)
        sigsqr, roots, ma, mu = cp.mle_to_model(x, p, q)
        # add_mle needs no sampler: it reads self.p, self.q and writes self.mle
        holder = types.SimpleNamespace(p=p, q=q, mle={})
        cp.CarmaSample.add_mle(holder, types.SimpleNamespace(x=x, fun=0.0))
        assert np.array_equal(roots, holder.mle["ar_roots"])
        assert np.array_equal(ma, np.atleast_1d(holder.mle["ma_coefs"]))
        assert mu == holder.mle["mu"] and roots.shape == (p,) and ma.shape == (q + 1,)
        assert abs(sigsqr - holder.mle["sigma"] ** 2) <= 4e-16 * sigsqr
        if p == 1:
            omega = np.exp(x[3])
            assert roots[0] == -omega and abs(sigsqr - 2.0 * omega * x[0] ** 2) <= 4e-16 * sigsqr
            continue
        oroots, oma = orc.ar_roots(x, p), orc.ma_coefs(x, p, q)[: q + 1]
        assert np.allclose(np.sort_complex(roots), np.sort_complex(oroots), rtol=1e-12, atol=0)
        assert np.allclose(ma, oma, rtol=1e-10, atol=1e-300)
        assert abs(sigsqr - x[0] ** 2 / orc.variance(oroots, oma)) <= 1e-9 * sigsqr


def test_mle_to_model_rejects_a_vector_of_the_wrong_order():
    with pytest.raises(ValueError):
        cp.mle_to_model(np.zeros(6), 3, 2)
    with pytest.raises(ValueError):
        cp.mle_to_model(np.zeros(4), 2, 0)
    with pytest.raises(ValueError):
        cp.mle_to_model(np.zeros(5), 2, 2)
    assert "mle_to_model" in cpa.__all__


def test_group_by_order():
    g = cp.group_by_order([(2, 0), (1, 0), (2, 0), (5, 3), (1, 0), (2, 1)])
    assert g == {(2, 0): [0, 2], (1, 0): [1, 4], (5, 3): [3], (2, 1): [5]}
    assert list(g) == [(2, 0), (1, 0), (5, 3), (2, 1)]


class _Recorder(object):
    """Stands in for a MultiContext: records the calls, returns arrays of the right shapes."""

    def __init__(self, n):
        self.n, self.calls = n, []

    def kfilter(self, which, sigsqr, roots, ma, mu=None):
        self.calls.append(("kfilter", list(which), np.shape(roots), np.shape(ma)))
        return ([np.zeros(self.n[s]) for s in which], [np.ones(self.n[s]) for s in which], np.zeros(len(which), dtype=bool))

    def predict(self, which, sigsqr, roots, ma, times, mu=None):
        self.calls.append(("predict", list(which), [np.asarray(t).size for t in times]))
        return [np.full(np.asarray(t).size, float(s)) for s, t in zip(which, times)], [np.ones(np.asarray(t).size) for t in times]


def _model_set(monkeypatch):
    ns = (20, 9, 33, 12, 5)
    series = []
    for k, n in enumerate(ns):
        t, y, e = irregular_series(n, 40 + k)
        series.append((t, y, e))
    ms = cp.CarmaModelSet(series, p=2, q=1)
    made = {}

    def context(p, q):
        return made.setdefault((p, q), _Recorder([m.time.size for m in ms.models]))
    monkeypatch.setattr(ms, "context", context)
    return ms, made


def _fits(ms, orders):
    rng = np.random.default_rng(5)
    out = []
    for m, (p, q) in zip(ms.models, orders):
        x = (np.array([1.0, 1.0, 0.3, -1.0]) if p == 1 else prior_like_theta(rng, p, q, m.time, m.y))
        out.append(cp.BatchResult(x, 0.0, 1, 1, True, ""))
    return out


def test_model_set_groups_by_order_one_call_per_order(monkeypatch):
    ms, made = _model_set(monkeypatch)
    orders = [(3, 2), (1, 0), (3, 2), (2, 1), (1, 0)]
    fits = _fits(ms, orders)
    mean, var = ms.predict(np.array([1.0, 2.0, 3.0]), fits, orders=orders)
    assert sorted(made) == [(1, 0), (2, 1), (3, 2)]
    assert made[(3, 2)].calls == [("predict", [0, 2], [3, 3])]
    assert made[(1, 0)].calls == [("predict", [1, 4], [3, 3])]
    assert made[(2, 1)].calls == [("predict", [3], [3])]
    assert [m[0] for m in mean] == [0.0, 1.0, 2.0, 3.0, 4.0] and all(v.shape == (3,) for v in var)
    out = ms.assess_fit(fits, orders=orders, nplot=7)
    assert [c[0] for c in made[(3, 2)].calls] == ["predict", "kfilter", "predict"]
    assert made[(3, 2)].calls[1] == ("kfilter", [0, 2], (2, 3), (2, 3))
    for s, d in enumerate(out):
        assert sorted(d) == ["mean", "resid_acf", "std_resid", "time", "var"]
        assert d["time"].shape == (7,) and d["time"][0] == ms.models[s].time.min() and d["time"][-1] == ms.models[s].time.max()
        assert d["std_resid"].shape == ms.models[s].time.shape and d["resid_acf"][0] == 1.0
    # orders default: self.orders of choose_order if set, else (self.p, self.q) for every series
    made.clear()
    ms.predict(0.5, _fits(ms, [(2, 1)] * 5))
    assert list(made) == [(2, 1)] and made[(2, 1)].calls == [("predict", [0, 1, 2, 3, 4], [1] * 5)]
    made.clear()
    ms.orders = orders
    ms.predict(0.5, fits)
    assert sorted(made) == [(1, 0), (2, 1), (3, 2)]


def test_model_set_predict_takes_one_array_or_a_list(monkeypatch):
    ms, made = _model_set(monkeypatch)
    fits = _fits(ms, [(2, 1)] * 5)
    ms.predict([0.5, 1.5], fits)                               # a plain list of numbers is ONE array of times
    assert made[(2, 1)].calls[-1] == ("predict", [0, 1, 2, 3, 4], [2] * 5)
    ms.predict([np.arange(k, dtype=float) for k in (4, 0, 1, 2, 3)], fits)
    assert made[(2, 1)].calls[-1] == ("predict", [0, 1, 2, 3, 4], [4, 0, 1, 2, 3])
    with pytest.raises(ValueError):
        ms.predict([np.arange(3.0)] * 4, fits)                 # a list, but not one per series


def test_model_set_argument_errors_come_before_any_library_call(monkeypatch):
    ms, made = _model_set(monkeypatch)
    fits = _fits(ms, [(2, 1)] * 5)
    for call in (lambda **kw: ms.predict(np.arange(3.0), **kw), lambda **kw: ms.assess_fit(**kw)):
        with pytest.raises(ValueError):
            call(fits=fits[:4])
        with pytest.raises(ValueError):
            call(fits=fits, orders=[(2, 1)] * 4)
        with pytest.raises(ValueError):
            call(fits=fits, orders=[(2, 2)] * 5)
        with pytest.raises(ValueError):
            call(fits=fits, orders=[(3, 1)] * 5)              # the vectors are CARMA(2,1) vectors: wrong length, series named
    assert not made


def test_null_and_bad_arguments_are_einval_without_a_device():
    x = np.zeros(8)
    dp = x.ctypes.data_as(C.POINTER(C.c_double))
    ip = np.zeros(2, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    lp = np.zeros(3, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_long))
    assert L.carma_mkfilter(None, ip, 1, dp, dp, dp, 1, None, dp, dp, None, None) == EINVAL
    assert L.carma_mpredict(None, ip, 1, dp, dp, dp, 1, None, dp, lp, dp, dp, None) == EINVAL
