"""The one-pass smoother -- carma_smooth_carma / carma_smooth_car1 / carma_msmooth, k_smooth_carma<P,G>, k_smooth_car1,
k_smooth_band -- and the Python layers on top (KalmanFilterp/1.SmoothBatch, CarmaSample.smooth / predict_band,
MultiContext.smooth, CarmaModelSet.smooth): the interpolated light curve at every order p = 1..7, at the launch edges of a
lane-group kernel (model counts on either side of a wave, chunk sizes), on series of one and two points, and the posterior band.

Yardsticks: the dense Gaussian-process conditional at 50 digits (mp_truth), the oracle's Predict only as the arbiter's other
side; for bits, the K = 1 call of the same model; for the band, the numpy mixture (tests/smooth_ref.py) of the call's own K x M
outputs."""
import os

import numpy as np
import pytest

import oracle as orc
import smooth_ref as sr
from helpers import (ROOT_KINDS, irregular_series, model_ma, model_roots, record_allowance, regrow_models, regrow_series)
from mp_truth import predict_truth, predict_truth_car1

pytestmark = pytest.mark.gpu

GROUP = {2: 2, 3: 4, 4: 4, 5: 8, 6: 8, 7: 8}          # lanes per model: GroupOf<P>
MODELS = [(p, q, kind) for p in range(2, 8) for q in (0, p - 1) for kind in (ROOT_KINDS if p > 2 else ROOT_KINDS[:2])]
MODEL_IDS = ["p%dq%d-%s" % m for m in MODELS]
EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    from carma_pack_amd import _lib
    assert _lib.lib.carma_device_count() >= 1
    return _lib


# (the helpers of tests/test_gpu_model_kernels.py, copied: the same models, series and rule)
def make_model(p, q, kind):
    """A well-conditioned model of the kind: cond of the variance sum (oracle.truth_variance) <= 1e4."""
    for attempt in range(20):
        rng = np.random.default_rng(100000 * attempt + 1000 * p + 10 * q + ROOT_KINDS.index(kind))
        roots, ma = model_roots(rng, p, kind), model_ma(rng, p, q)
        v, cond = orc.truth_variance(roots, ma, with_cond=True)
        if cond <= 1e4:
            return roots, ma, v
    raise AssertionError("no well-conditioned model for %r" % ((p, q, kind),))


def centred_series(n, seed, v1):
    t, y, yerr = irregular_series(n, seed)
    y = y - y.mean()
    return t, y, yerr, float(np.var(y) / v1)


def assert_near_truth(got_m, got_v, tm, tv, om, ov, what, rtol=1e-9):
    """Smoothed moments against the exact (50-digit) values: variances to rtol relative, means to rtol of max(|mean|, sd).  An
    entry beyond rtol passes only where the oracle misses rtol as well and the device is no further from the exact value than
    the oracle is; every such entry is counted (record_allowance)."""
    got_m, got_v = np.asarray(got_m), np.asarray(got_v)
    assert np.all(np.isfinite(got_m)) and np.all(np.isfinite(got_v)), what
    sm = np.maximum(np.abs(tm), np.sqrt(tv))
    nb = 0
    for g, o, tr, sc, name in ((got_m, om, tm, sm, "mean"), (got_v, ov, tv, tv, "var")):
        eg, eo = np.abs(g - tr) / sc, np.abs(o - tr) / sc
        bad = np.flatnonzero(eg > rtol)
        for i in bad:
            assert eo[i] > rtol and eg[i] <= eo[i], "%s: %s[%d] %.3e from the exact value (oracle %.3e)" % (
                what, name, i, eg[i], eo[i])
        nb += bad.size
    record_allowance("smooth: device beyond %.0e of the 50-digit value, no further than the oracle" % rtol, what, nb, nb,
                     2 * got_m.size)


def special_times(t, rng, count):
    far_back, far_fore = t[0] - 5000.0, t[-1] + 5000.0
    special = [far_back, t[0] - 2.5, t[0], t[1], t[7], t[24], t[-1], 0.5 * (t[3] + t[4]), 0.5 * (t[-2] + t[-1]),
               t[-1] + 1.5, far_fore]
    special += [special[4], special[7]]                                   # repeated times
    tp = rng.permutation(np.r_[special, rng.uniform(t[0] - 8.0, t[-1] + 8.0, count - len(special))])
    return tp, far_back, far_fore, (special[4], special[7])


def one(lib, t, y, yerr, sigsqr, roots, ma, tp, mu=None):
    m, v = lib.smooth_carma(t, y, yerr, [sigsqr], np.asarray(roots)[None, :], np.asarray(ma)[None, :], mu, tp)
    return m[0], v[0]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q,kind", MODELS, ids=MODEL_IDS)
def test_truth_at_every_order(lib, p, q, kind):
    """k_smooth_carma<P,G>, K = 1, on the inputs of the predict test: backcasts far and near, exactly t[0] and interior data
    times, midpoints, repeated and unsorted times, forecasts near and far."""
    import carma_pack_amd as cpa
    roots, ma, v1 = make_model(p, q, kind)
    t, y, yerr, sigsqr = centred_series(48, 70 + 10 * p + q, v1)
    rng = np.random.default_rng(900 + 10 * p + q)
    tp, far_back, far_fore, rep = special_times(t, rng, 25)
    tm, tv = predict_truth(t, y, yerr, sigsqr, roots, ma, tp)
    om, ov = orc.predict_carma(t, y, yerr, sigsqr, roots, ma, tp)
    what = "smooth p=%d q=%d %s" % (p, q, kind)
    pm, pv = one(lib, t, y, yerr, sigsqr, roots, ma, tp)
    assert_near_truth(pm, pv, tm, tv, om, ov, what)
    v0 = cpa.carma_variance(sigsqr, roots, ma)
    for far in (far_back, far_fore):
        i = int(np.flatnonzero(tp == far)[0])
        assert abs(pm[i]) <= 1e-12 * np.sqrt(v0), (what, far, pm[i])
        assert abs(pv[i] - v0) <= 1e-9 * v0, (what, far, pv[i], v0)
    for x in rep:
        i = np.flatnonzero(tp == x)
        assert i.size >= 2 and np.all(pm[i] == pm[i[0]]) and np.all(pv[i] == pv[i[0]]), (what, x)


@pytest.mark.parametrize("p", (2, 3, 5, 7))
def test_launch_edges_and_chunks(lib, p):
    """K = 1, E - 1, E, E + 1, 3 E + 1 models (E = 64 / G per wave), three distinct ones cycled with distinct mu: every row has
    the bits of the K = 1 call of its model, also with the chunk size forced to 1 and to E + 1."""
    q = p - 1
    E = 64 // GROUP[p]
    kinds = ("complex", "mixed", "real") if p > 2 else ("complex", "real", "complex")
    mods = [make_model(p, q if k != 2 else 0, kinds[k]) for k in range(3)]
    t, y, yerr = irregular_series(48, 40 + p)
    y = y + 2.0
    mus = np.array([1.9, 2.0, 2.15])
    sigs = np.array([np.var(y) / m[2] for m in mods])
    tp = special_times(t, np.random.default_rng(p), 20)[0]
    alone = [one(lib, t, y, yerr, sigs[k], mods[k][0], mods[k][1], tp, mu=mus[k:k + 1]) for k in range(3)]
    assert not np.array_equal(alone[0][0], alone[1][0])

    def check(K, what):
        idx = np.arange(K) % 3
        m, v = lib.smooth_carma(t, y, yerr, sigs[idx], np.array([mods[k][0] for k in idx]), np.array([mods[k][1] for k in idx]),
                                mus[idx], tp)
        for i, k in enumerate(idx):
            assert np.array_equal(m[i], alone[k][0]) and np.array_equal(v[i], alone[k][1]), (p, what, K, i)

    for K in (1, E - 1, E, E + 1, 3 * E + 1):
        check(K, "automatic")
    try:
        for c in (1, E + 1):
            lib.tune_set("SMOOTH_CHUNK_MODELS", c)
            for K in (1, E - 1, E, E + 1, 3 * E + 1):
                check(K, "chunk %d" % c)
    finally:
        lib.tune_set("SMOOTH_CHUNK_MODELS", None)


@pytest.mark.parametrize("p", range(2, 8))
def test_series_edges(lib, p):
    """n = 1, n = 2, a series whose times all collapse to one, an unsorted one with duplicates (the bits of the call on
    oracle.sort_dedup's output, the exact values of the deduplicated series), M = 1, and requested times that are all data times."""
    kind = "mixed" if p > 2 else "complex"
    roots, ma, v1 = make_model(p, p - 1, kind)
    t, y, yerr, sigsqr = centred_series(24, 40 + p, v1)
    rng = np.random.default_rng(60 + p)
    perm = rng.permutation(t.size)
    cases = {
        "n=1": (t[:1], y[:1], yerr[:1]),
        "n=2": (t[:2], y[:2], yerr[:2]),
        "one time": (np.full(4, t[3]), y[3:7], yerr[3:7]),
        "unsorted with duplicates": (np.r_[t[perm], t[2], t[9], t[9]], np.r_[y[perm], 3.0, -2.0, 1.0],
                                     np.r_[yerr[perm], 0.7, 0.2, 0.4]),
    }
    tp = np.r_[t[0] - 40.0, t[0] - 1.0, t[0], t[0] + 0.4, t[1], t[1] + 2.0, t[3], t[9], t[-1] + 3.0]
    for name, (tt, yy, ee) in cases.items():
        ts, ys, es = orc.sort_dedup(tt, yy, ee)
        pm, pv = one(lib, tt, yy, ee, sigsqr, roots, ma, tp)
        pm2, pv2 = one(lib, ts, ys, es, sigsqr, roots, ma, tp)
        assert np.array_equal(pm, pm2) and np.array_equal(pv, pv2), (p, name)
        tm, tv = predict_truth(ts, ys, es, sigsqr, roots, ma, tp)
        om, ov = orc.predict_carma(ts, ys, es, sigsqr, roots, ma, tp)
        assert_near_truth(pm, pv, tm, tv, om, ov, "smooth p=%d %s" % (p, name))
    for name, tq in (("M=1", tp[3:4]), ("data times", t[[5, 0, 23, 5, 11]])):
        pm, pv = one(lib, t, y, yerr, sigsqr, roots, ma, tq)
        tm, tv = predict_truth(t, y, yerr, sigsqr, roots, ma, tq)
        om, ov = orc.predict_carma(t, y, yerr, sigsqr, roots, ma, tq)
        assert_near_truth(pm, pv, tm, tv, om, ov, "smooth p=%d %s" % (p, name))


@pytest.mark.parametrize("p", (5, 7))
def test_one_long_pass(lib, p):
    """n = 270, M = 32: the recursion's length in one pass, against the exact conditional."""
    roots, ma, v1 = make_model(p, p - 1, "mixed")
    t, y, yerr, sigsqr = centred_series(270, 500 + p, v1)
    tp = np.random.default_rng(p).uniform(t[0] - 5.0, t[-1] + 5.0, 32)
    tm, tv = predict_truth(t, y, yerr, sigsqr, roots, ma, tp)
    om, ov = orc.predict_carma(t, y, yerr, sigsqr, roots, ma, tp)
    pm, pv = one(lib, t, y, yerr, sigsqr, roots, ma, tp)
    assert_near_truth(pm, pv, tm, tv, om, ov, "smooth long p=%d" % p)


@pytest.mark.parametrize("p", (3, 5, 7))
def test_high_signal_to_noise(lib, p):
    """yerr x 1e-2: the variance f - u^H N u cancels (the smoothed variance is ~3e-6 of var(y)).  The device is at most 8 x as
    far from the exact value as the numpy restatement on the same input (another summation order, the table exp), or 1e-9:
    worst entry against worst entry, means and variances each."""
    roots, ma, v1 = make_model(p, p - 1, "mixed")
    t, y, yerr, sigsqr = centred_series(48, 70 + 11 * p, v1)
    yerr = 1e-2 * yerr
    tp = special_times(t, np.random.default_rng(p), 25)[0]
    tm, tv = predict_truth(t, y, yerr, sigsqr, roots, ma, tp)
    rm, rv = sr.smooth_carma(t, y, yerr, sigsqr, roots, ma, tp)
    pm, pv = one(lib, t, y, yerr, sigsqr, roots, ma, tp)
    assert np.all(np.isfinite(pm)) and np.all(np.isfinite(pv))
    sm = np.maximum(np.abs(tm), np.sqrt(tv))
    worst = 0.0
    for g, r, tr, sc, name in ((pm, rm, tm, sm, "mean"), (pv, rv, tv, tv, "var")):
        eg, er = np.abs(g - tr) / sc, np.abs(r - tr) / sc
        print("high S/N p=%d %s: device %.2e, restatement %.2e from the exact value" % (p, name, eg.max(), er.max()))
        bound = max(8.0 * er.max(), 1e-9)
        assert eg.max() <= bound, (p, name, eg.max(), er.max())
        worst = max(worst, eg.max() / max(er.max(), 1e-300))
    record_allowance("smooth at high S/N: device within 8 x the restatement's distance from the exact value (ratio %.2f)" % worst,
                     "p=%d" % p, 0, 0, 2 * tp.size)


def test_car1_at_lane_counts(lib):
    """k_smooth_car1 (one lane per model) at K = 1, 63, 64, 65, 200 against the 50-digit CAR(1) conditional; a row does not
    depend on its batch."""
    t, y, yerr = irregular_series(60, 31)
    y = y - y.mean()
    rng = np.random.default_rng(32)
    tp = rng.permutation(np.r_[t[0] - 4000.0, t[0] - 3.0, t[0], t[5], t[-1], 0.5 * (t[8] + t[9]), t[-1] + 2.0, t[5], t[-1] + 4000.0,
                               rng.uniform(t[0] - 5.0, t[-1] + 5.0, 11)])
    omegas = np.array([0.04, 0.7])
    truth = [predict_truth_car1(t, y, yerr, 2.0 * o * np.var(y), o, tp) for o in omegas]
    orac = [orc.predict_car1(t, y, yerr, 2.0 * o * np.var(y), o, tp) for o in omegas]
    alone = [lib.smooth_car1(t, y, yerr, [2.0 * o * np.var(y)], [o], None, tp) for o in omegas]
    for K in (1, 63, 64, 65, 200):
        om = omegas[np.arange(K) % 2]
        m, v = lib.smooth_car1(t, y, yerr, 2.0 * om * np.var(y), om, None, tp)
        assert m.shape == (K, tp.size)
        for i in range(K):
            assert np.array_equal(m[i], alone[i % 2][0][0]) and np.array_equal(v[i], alone[i % 2][1][0]), (K, i)
        for k in range(min(K, 2)):
            assert_near_truth(m[k], v[k], truth[k][0], truth[k][1], orac[k][0], orac[k][1], "smooth car1 omega=%g K=%d" % (omegas[k], K))
    # mu: subtracted from the data, added back to the mean
    m2, v2 = lib.smooth_car1(t, y + 3.0, yerr, [2.0 * 0.7 * np.var(y)], [0.7], [3.0], tp)
    assert np.allclose(m2[0] - 3.0, alone[1][0][0], rtol=0, atol=1e-12) and np.allclose(v2[0], alone[1][1][0], rtol=1e-13)


# ---------------------------------------------------------------------------------------------------------------------
# the band

def _band_models(p, K, seed):
    q = min(1, p - 1)
    kinds = ("complex", "mixed") if p > 2 else ("complex", "real")
    rng = np.random.default_rng(seed)
    roots = np.array([model_roots(rng, p, kinds[k % 2]) for k in range(K)])
    ma = np.array([model_ma(rng, p, q)[:q + 1] for k in range(K)])
    return rng.uniform(0.5, 2.0, K), roots, ma, rng.normal(0.0, 0.1, K)


def _assert_band(bm, bv, m, v, keep=None):
    """4 K 2^-53 of the sum of |terms| per entry: the bound of a K-term ordered sum."""
    rm, rvv, am, av = sr.band_moments(m, v, keep)
    K = m.shape[0] if keep is None else int(np.sum(keep))
    eps = 4.0 * K * 2.0 ** -53
    assert np.all(np.abs(bm - rm) <= eps * am), np.max(np.abs(bm - rm) / am)
    # (the two sides' band means differ by rounding; the deviations from the mean sum to zero, so that moves the sum of their
    # squares in second order only)
    assert np.all(np.abs(bv - rvv) <= eps * av), np.max(np.abs(bv - rvv) / av)


@pytest.mark.parametrize("K", (1, 5, 67))
def test_band_is_the_mixture_of_the_calls_own_rows(lib, K):
    p = 3
    t, y, yerr = irregular_series(40, 77)
    sig, roots, ma, mu = _band_models(p, K, 10 + K)
    tp = special_times(t, np.random.default_rng(K), 25)[0]
    m, v, bm, bv = lib.smooth_carma(t, y, yerr, sig, roots, ma, mu, tp, band=True)
    assert m.shape == (K, 25) and bm.shape == (25,)
    if K == 1:
        assert np.array_equal(bm, m[0]) and np.array_equal(bv, v[0])
    _assert_band(bm, bv, m, v)
    # band only: the same bits, and the rows are those of a call without the band
    bm2, bv2 = lib.smooth_carma(t, y, yerr, sig, roots, ma, mu, tp, band="only")
    assert np.array_equal(bm2, bm) and np.array_equal(bv2, bv)
    m3, v3 = lib.smooth_carma(t, y, yerr, sig, roots, ma, mu, tp)
    assert np.array_equal(m3, m) and np.array_equal(v3, v)
    # CAR(1)
    om = np.random.default_rng(K).uniform(0.03, 0.8, K)
    m, v, bm, bv = lib.smooth_car1(t, y, yerr, 2.0 * om * np.var(y), om, mu, tp, band=True)
    _assert_band(bm, bv, m, v)
    assert all(np.array_equal(a, b) for a, b in zip(lib.smooth_car1(t, y, yerr, 2.0 * om * np.var(y), om, mu, tp, band="only"),
                                                    (bm, bv)))


def test_band_leaves_a_singular_model_out(lib):
    t, y, yerr = irregular_series(40, 3)
    sig, roots, ma, mu = _band_models(3, 5, 9)
    tp = np.linspace(t[0] - 3.0, t[-1] + 3.0, 7)
    good = lib.smooth_carma(t, y, yerr, sig, roots, ma, mu, tp, band=True, return_singular=True)
    assert not good[4].any()
    bad = roots.copy()
    bad[2] = [-0.5, -0.5, -0.2]                                          # a repeated AR root
    m, v, bm, bv, flags = lib.smooth_carma(t, y, yerr, sig, bad, ma, mu, tp, band=True, return_singular=True)
    assert flags.tolist() == [False, False, True, False, False]
    keep = ~flags
    assert np.array_equal(m[keep], good[0][keep]) and np.array_equal(v[keep], good[1][keep])
    _assert_band(bm, bv, m, v, keep)                                      # K' = 4
    four = lib.smooth_carma(t, y, yerr, sig[keep], roots[keep], ma[keep], mu[keep], tp, band="only")
    assert np.array_equal(four[0], bm) and np.array_equal(four[1], bv)
    with pytest.raises(lib.CarmaError, match="model 2"):
        lib.smooth_carma(t, y, yerr, sig, bad, ma, mu, tp)


def test_argument_errors_leave_the_library_usable(lib):
    """Roots not closed under conjugation, nma outside 1..p and K < 1: CARMA_EINVAL with the index; the next call is good."""
    import ctypes as C
    t, y, yerr = irregular_series(30, 4)
    sig, roots, ma, mu = _band_models(3, 4, 5)
    tp = np.linspace(t[0], t[-1], 6)
    good = lib.smooth_carma(t, y, yerr, sig, roots, ma, mu, tp)
    om = lambda r: np.ascontiguousarray(np.stack([r.real, r.imag], axis=-1))      # noqa: E731
    out = np.zeros((4, 6))

    def raw(K, r, nma):
        return lib.lib.carma_smooth_carma(lib.ptr(t), lib.ptr(y), lib.ptr(yerr), t.size, 3, K, lib.ptr(sig), lib.ptr(om(r)),
                                          lib.ptr(np.ascontiguousarray(ma)), nma, lib.ptr(mu), lib.ptr(tp), 6, lib.ptr(out),
                                          lib.ptr(out.copy()), None, None, None, None, lib.default_device())

    open_roots = roots.copy()
    open_roots[3] = [-0.1 - 0.5j, -0.1 + 0.4j, -0.3]
    assert raw(4, open_roots, 2) == EINVAL and "model 3" in lib.last_error()
    for nma in (0, 4):
        assert raw(4, roots, nma) == EINVAL and "nma" in lib.last_error()
    for K in (0, -2):
        assert raw(K, roots, 2) == EINVAL and "nmodels" in lib.last_error()
    assert np.all(out == 0.0)
    with pytest.raises(ValueError):
        lib.smooth_carma(t, y, yerr, sig, open_roots, ma, mu, tp)
    again = lib.smooth_carma(t, y, yerr, sig, roots, ma, mu, tp)
    assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1])
    del C


# ---------------------------------------------------------------------------------------------------------------------
# the set form

@pytest.mark.parametrize("p,q", [(2, 1), (5, 1), (1, 0)])
def test_set_items_have_the_bits_of_the_one_series_call(lib, p, q):
    """carma_msmooth on the series of 20, 33 and 70 points: items that share a series and a list of times (more than a wave of
    them), items that do not, an item without times; a small, a large and a small call on one context equal fresh ones."""
    series = [(t, y + 1.5, e) for t, y, e in regrow_series()]
    E = 64 if p == 1 else 64 // GROUP[p]
    M = E + 7
    sig, roots, ma = regrow_models(p, q, M, 60 + 10 * p + q)
    if p == 1:
        roots = roots[:, 0]
    rng = np.random.default_rng(70 + p)
    mu = 1.5 + rng.normal(0.0, 0.05, M)
    shared = np.r_[-30.0, rng.uniform(-5.0, 120.0, 9), 4000.0, series[2][0][[4, 0]]]
    which = np.r_[np.full(E + 2, 2), 0, 1, 1, 0, 2][:M]
    times = [shared] * (E + 2) + [shared[:3], shared, np.array([]), rng.uniform(0.0, 40.0, 5), shared[::-1]]
    times = times[:M]
    ctx = lib.MultiContext(series, p, q)
    pm, pv = ctx.smooth(which, sig, roots, ma, times, mu=mu)
    assert [a.size for a in pm] == [x.size for x in times]
    for i in range(M):
        if times[i].size == 0:
            continue
        t, y, e = series[which[i]]
        if p == 1:
            sm, sv = lib.smooth_car1(t, y, e, sig[i:i + 1], -roots[i:i + 1].real, mu[i:i + 1], times[i])
        else:
            sm, sv = lib.smooth_carma(t, y, e, sig[i:i + 1], roots[i:i + 1], ma[i:i + 1], mu[i:i + 1], times[i])
        assert np.array_equal(pm[i], sm[0]) and np.array_equal(pv[i], sv[0]), (p, i)
    # ... and with the waves of the call cut into chunks
    try:
        lib.tune_set("SMOOTH_CHUNK_MODELS", 1)
        pm2, pv2 = ctx.smooth(which, sig, roots, ma, times, mu=mu)
    finally:
        lib.tune_set("SMOOTH_CHUNK_MODELS", None)
    assert all(np.array_equal(a, b) for a, b in zip(pm + pv, pm2 + pv2))
    # buffer regrowth: small, large, small on one context, each equal to a fresh context's
    for idx in (np.arange(2), np.arange(M), np.arange(2)):
        sub = lambda c: c.smooth(which[idx], sig[idx], roots[idx], ma[idx], [times[i] for i in idx], mu=mu[idx])   # noqa: E731
        fresh = lib.MultiContext(series, p, q)
        got, want = sub(ctx), sub(fresh)
        fresh.close()
        assert all(np.array_equal(a, b) for a, b in zip(got[0] + got[1], want[0] + want[1])), (p, idx.size)
        assert all(np.array_equal(got[0][k], pm[i]) for k, i in enumerate(idx))
    # errors name their item and leave the context usable
    bad = [x.copy() for x in times]
    bad[1] = np.r_[bad[1][:2], np.inf]
    with pytest.raises(ValueError, match="item 1"):
        ctx.smooth(which, sig, roots, ma, bad, mu=mu)
    with pytest.raises(ValueError):
        ctx.smooth(which, sig, roots, ma, times[:-1], mu=mu)
    a, b = ctx.smooth(which[:3], sig[:3], roots[:3], ma[:3], times[:3], mu=mu[:3])
    assert all(np.array_equal(a[k], pm[k]) and np.array_equal(b[k], pv[k]) for k in range(3))
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# the Python API

@pytest.fixture(scope="module")
def samples(golden_dir):
    import carmcmc as cm
    g = np.load(os.path.join(golden_dir, "carma53_readme.npz"))
    t, y, e = g["t"][:60], g["y"][:60], g["yerr"][:60]
    s31 = cm.CarmaModel(t, y, e, p=3, q=1).run_mcmc(200, nburnin=100, seed=5)
    s1 = cm.CarmaModel(t, y, e, p=1).run_mcmc(200, nburnin=100, seed=5)
    return cm, t, y, e, {3: s31, 1: s1}


@pytest.mark.parametrize("p", [3, 1])
def test_sample_smooth_and_predict_band(lib, samples, p):
    cm, t, y, e, ss = samples
    sample = ss[p]
    ts = np.r_[t[0] - 3.0, np.linspace(t[0], t[-1], 9), t[4], t[-1] + 2.0]
    pm, pv = sample.predict(ts, "map")
    sm, sv = sample.smooth(ts, "map")
    assert np.max(np.abs(sm - pm) / np.maximum(np.abs(pm), np.sqrt(pv))) <= 1e-9 and np.max(np.abs(sv - pv) / pv) <= 1e-9
    a, b = sample.smooth(float(ts[3]), 17)
    c, d = sample.smooth(ts[3:4], 17)
    assert np.isscalar(a) and a == c[0] and b == d[0]
    kf, mu = sample.makeKalmanFilter("map")
    k1, k2 = kf.SmoothBatch(cm.vecD(ts.tolist()))
    assert np.array_equal(k1 + mu, sm) and np.array_equal(k2, sv)
    # the band: reproducible, the mixture of its own samples, and the band-only call's bits
    bm, bv, m, v, idx = sample.predict_band(ts, nsamples=40, seed=3, return_samples=True)
    assert m.shape == (40, ts.size) and idx.shape == (40,) and len(set(idx.tolist())) == 40 and np.all((idx >= 0) & (idx < 200))
    again = sample.predict_band(ts, nsamples=40, seed=3, return_samples=True)
    assert all(np.array_equal(x, z) for x, z in zip(again, (bm, bv, m, v, idx)))
    assert not np.array_equal(sample.predict_band(ts, nsamples=40, seed=4, return_samples=True)[4], idx)
    _assert_band(bm, bv, m, v)
    only = sample.predict_band(ts, nsamples=40, seed=3)
    assert np.array_equal(only[0], bm) and np.array_equal(only[1], bv)
    for j in (0, 39):                                                    # row j is sample idx[j]'s curve
        rm, rv = sample.smooth(ts, int(idx[j]))
        assert np.allclose(m[j], rm, rtol=0, atol=1e-9 * np.sqrt(rv).max()) and np.allclose(v[j], rv, rtol=1e-9)
    # without a seed: the evenly spaced samples of the spectrum plots; all samples by default
    assert np.array_equal(sample.predict_band(ts, nsamples=10, return_samples=True)[4], sample._subsample(10, 200))
    full = sample.predict_band(ts)
    assert full[0].shape == ts.shape and np.all(np.isfinite(full[0])) and np.all(full[1] > 0)


def test_model_set_smooth_is_a_loop_over_sample_smooth(lib):
    """CarmaModelSet.smooth against KalmanFilterp / KalmanFilter1.SmoothBatch of the same mle_to_model models, bit for bit,
    and against predict to 1e-9."""
    import carmcmc as cm
    orders = [(1, 0), (2, 0), (3, 2), (2, 0)]
    series = []
    for k, n in enumerate((40, 33, 64, 21)):
        t, y, e = irregular_series(n, 950 + k)
        series.append((t, y + 2.0, e))
    ms = cm.CarmaModelSet(series, p=2, q=0)
    rng = np.random.default_rng(951)
    fits = []
    for m, (p, q) in zip(ms.models, orders):
        if p == 1:
            fits.append(np.array([np.std(m.y), 1.0, m.y.mean(), np.log(0.2)]))
        else:
            from helpers import prior_like_theta
            fits.append(prior_like_theta(rng, p, q, m.time, m.y))
    tgrid = np.r_[-30.0, np.linspace(0.0, 40.0, 9), 4000.0]
    sm, sv = ms.smooth(tgrid, fits, orders=orders)
    pm, pv = ms.predict(tgrid, fits, orders=orders)
    sl, _ = ms.smooth([tgrid[:s + 1] for s in range(4)], fits, orders=orders)
    for s, (m, (p, q)) in enumerate(zip(ms.models, orders)):
        sigsqr, roots, ma, mu = cm.mle_to_model(fits[s], p, q)
        tv, yv, ev = cm.vecD(m.time.tolist()), cm.vecD((m.y - mu).tolist()), cm.vecD(m.ysig.tolist())
        if p == 1:
            kf = cm.KalmanFilter1(tv, yv, ev, sigsqr, float(-roots[0].real))
        else:
            kf = cm.KalmanFilterp(tv, yv, ev, sigsqr, cm.vecC([complex(r) for r in roots]), cm.vecD(ma.tolist()))
        a, b = kf.SmoothBatch(tgrid)
        sc = np.maximum(np.abs(pm[s] - mu), np.sqrt(pv[s]))
        assert np.max(np.abs(sm[s] - pm[s]) / sc) <= 1e-9 and np.max(np.abs(sv[s] - pv[s]) / pv[s]) <= 1e-9, (s, p, q)
        # (the set subtracts mu on the device, the one-series object gets centred data: the same subtraction, the same bits)
        assert np.array_equal(sm[s], a + mu) and np.array_equal(sv[s], b), (s, p, q)
        assert np.array_equal(sl[s], sm[s][:s + 1])
