"""Filter and predict of every light curve of a set in one launch: carma_mkfilter / carma_mpredict (MultiContext.kfilter /
predict) and CarmaModelSet.assess_fit / predict on top of them.

The filter runs one (series, model) item per lane with a series pointer and a length of the lane's own, so the cases sit where
that can go wrong: series of 2 ... 270 points mixed in one wave, item counts on either side of a wave, several items on one
series and a series without any, a regular-cadence series (repeated time steps) next to irregular ones.  Yardsticks: the
one-series entry points, bit for bit (same device functions); the oracle under the rule of test_batched_filter_at_tile_edges;
the 50-digit conditional for predict."""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
from helpers import (REGROW_ORDERS, assert_all_equal, irregular_series, prior_like_theta, record_allowance, regrow_models,
                     regrow_series)
from mp_truth import predict_truth, predict_truth_car1
from test_gpu_model_kernels import GROUP, REPEATED_ROOTS, assert_near_truth, make_model

pytestmark = pytest.mark.gpu

EINVAL = -22
_dp, _ip, _lp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_long)


@pytest.fixture(scope="module")
def lib():
    from carma_pack_amd import _lib
    assert _lib.lib.carma_device_count() >= 1
    return _lib


def filter_set():
    """12 series, uncentred (y + 3): n in {2, 3, 31, 63, 64, 65, 130, 270}, one regular-cadence series, one unsorted with
    duplicate times, and (last) one that the tests give no item."""
    series = []
    for k, n in enumerate((2, 3, 31, 63, 64, 65, 130, 270, 65, 31)):
        t, y, e = irregular_series(n, 800 + k)
        series.append((t, y + 3.0, e))
    t, y, e = irregular_series(90, 820)
    series.append((np.arange(90.0) * 0.75, y + 3.0, e))                       # regular cadence: every step repeats its predecessor
    t, y, e = irregular_series(40, 821)
    perm = np.random.default_rng(822).permutation(43)
    series.append((np.r_[t, t[4], t[17], t[17]][perm], np.r_[y, 1.0, -2.0, 0.5][perm] + 3.0, np.r_[e, 0.3, 0.6, 0.2][perm]))
    t, y, e = irregular_series(50, 823)
    series.append((t, y + 3.0, e))                                            # no item
    return series


def models_for(p, q, count, seed):
    """`count` prior-like models as test_batched_filter_at_tile_edges draws them: (theta, roots, ma [q + 1], sigsqr)."""
    rng = np.random.default_rng(seed)
    t0, y0, _ = irregular_series(65, 300 + p)
    th = np.array([prior_like_theta(rng, p, q, t0, y0) for _ in range(count)])
    roots = np.array([orc.ar_roots(x, p) for x in th])
    ma = np.array([orc.ma_coefs(x, p, q) for x in th])[:, : q + 1]
    sig2 = np.array([x[0] ** 2 / orc.variance(r, m) for x, r, m in zip(th, roots, ma)])
    return th, roots, ma, sig2


def raw_kfilter(lib, ctx, which, sig, roots, ma, mu, pad=8, sentinel=-7.25, M=None, nma=None):
    """carma_mkfilter through ctypes with output buffers `pad` doubles longer than the items need, filled with a sentinel.
    Returns (rc, mean, var, offsets, singular, total)."""
    which = np.ascontiguousarray(which, dtype=np.int32)
    sig = np.ascontiguousarray(sig, dtype=np.float64)
    roots = np.asarray(roots, dtype=complex)
    om = np.ascontiguousarray(np.stack([roots.real, roots.imag], axis=-1))
    ma = np.ascontiguousarray(ma, dtype=np.float64)
    mu = np.ascontiguousarray(mu, dtype=np.float64)
    total = int(sum(ctx.n[w] for w in which if 0 <= w < ctx.nseries))
    mean, var = np.full(total + pad, sentinel), np.full(total + pad, sentinel)
    off = np.zeros(which.size + 1, dtype=np.int64)
    sing = np.zeros(which.size, dtype=np.int32)
    rc = lib.lib.carma_mkfilter(ctx.handle, which.ctypes.data_as(_ip), which.size if M is None else M, sig.ctypes.data_as(_dp),
                                om.ctypes.data_as(_dp), ma.ctypes.data_as(_dp), ma.shape[1] if nma is None else nma,
                                mu.ctypes.data_as(_dp), mean.ctypes.data_as(_dp), var.ctypes.data_as(_dp), off.ctypes.data_as(_lp),
                                sing.ctypes.data_as(_ip))
    return rc, mean, var, off, sing, total


# ---------------------------------------------------------------------------------------------------------------------
# filter

@pytest.mark.parametrize("p,q", [(p, q) for p in range(2, 8) for q in (0, p - 1)])
def test_filter_items_against_the_one_series_path(lib, p, q):
    """k_mkfilter_carma_lane<P> + k_mtranspose_mv: 130 items spread over 12 series of 2 ... 270 points, M in {1, 63, 64, 65,
    130}.  Every item's rows are the bits kfilter_carma_batch gives for that model on that series alone with the same mu, and
    agree with the oracle under the rule of test_batched_filter_at_tile_edges: 1e-9, or no further from the quad-precision
    filter than 1.25 x the oracle, for at most 10 % of the items."""
    series = filter_set()
    S = len(series)
    ctx = lib.MultiContext(series, p, q)
    th, roots, ma, sig2 = models_for(p, q, 130, 7100 + 10 * p + q)
    rng = np.random.default_rng(7200 + 10 * p + q)
    which = np.r_[7, rng.permutation(np.arange(129) % (S - 1))]               # item 0 on the longest series; the last series: none
    data = [orc.sort_dedup(*s) for s in series]
    mu = np.array([data[w][1].mean() for w in which]) + rng.normal(0.0, 0.05, 130)
    assert [d[0].size for d in data] == list(ctx.n)
    alone = []
    for i in range(130):
        t, y, e = data[which[i]]
        m1, v1, s1 = lib.kfilter_carma_batch(t, y, e, sig2[i:i + 1], roots[i:i + 1], ma[i:i + 1], mu=mu[i:i + 1])
        assert not s1.any()
        alone.append((m1[0], v1[0]))
    for M in (130, 1, 63, 64, 65):
        means, vars_, sing = ctx.kfilter(which[:M], sig2[:M], roots[:M], ma[:M], mu=mu[:M])
        assert len(means) == M and len(vars_) == M and not sing.any(), (p, q, M)
        for i in range(M):
            assert means[i].shape == (ctx.n[which[i]],), (p, q, M, i)
            assert np.array_equal(means[i], alone[i][0]) and np.array_equal(vars_[i], alone[i][1]), (p, q, M, i, which[i])
    nworse = 0
    for i in range(130):
        t, y, e = data[which[i]]
        yc = y - mu[i]
        om, ov = orc.kfilter_carma(t, yc, e, sig2[i], roots[i], ma[i])
        sc = np.abs(yc).max()
        gm, gv = alone[i][0] - mu[i], alone[i][1]
        d_dev = max(np.max(np.abs(gm - om)) / sc, np.max(np.abs(gv - ov) / ov))
        if d_dev > 1e-9:
            thx = th[i].copy()
            thx[1], thx[2] = 1.0, 0.0
            tm, tv = orc.truth_filter(t, yc, e, thx, p, q)
            eo = max(np.max(np.abs(om - tm)) / sc, np.max(np.abs(ov - tv) / tv))
            eg = max(np.max(np.abs(gm - tm)) / sc, np.max(np.abs(gv - tv) / tv))
            print("p=%d q=%d item %d series %d: device %.3e oracle %.3e from the quad-precision filter" % (p, q, i, which[i], eg, eo))
            assert eg <= max(1e-9, 1.25 * eo), (p, q, i, eg, eo)
            nworse += 1
    assert nworse <= 0.1 * 130, (nworse, 130)
    if nworse:
        record_allowance("set filter: beyond 1e-9, no further from the quad-precision filter than 1.25 x the oracle",
                         "p=%d q=%d" % (p, q), nworse, 13, 130)


@pytest.mark.parametrize("p", (3, 6))
def test_filter_item_is_independent_of_its_batch(lib, p):
    """An item's rows are the same bits in the full batch, alone and in permuted batches (the plan sorts by length: every
    permutation lands an item in another lane next to other lengths); the output buffers are untouched past the last item's
    n_i, whichever item comes last -- the shortest series (n = 2), the longest (270), any."""
    q = p - 1
    series = filter_set()
    S = len(series)
    ctx = lib.MultiContext(series, p, q)
    _, roots, ma, sig2 = models_for(p, q, 70, 7300 + p)
    rng = np.random.default_rng(7400 + p)
    which = np.r_[rng.permutation(np.arange(68) % (S - 1)), 0, 7]
    mu = rng.normal(3.0, 0.1, 70)
    rc, mean, var, off, sing, total = raw_kfilter(lib, ctx, which, sig2, roots, ma, mu)
    assert rc == 0 and not sing.any() and off[-1] == total and np.array_equal(np.diff(off), ctx.n[which])
    assert np.all(mean[total:] == -7.25) and np.all(var[total:] == -7.25) and not np.any(mean[:total] == -7.25)
    full = [(mean[off[i]:off[i + 1]].copy(), var[off[i]:off[i + 1]].copy()) for i in range(70)]
    for i in (0, 5, 68, 69):
        m1, v1, _ = ctx.kfilter(which[i:i + 1], sig2[i:i + 1], roots[i:i + 1], ma[i:i + 1], mu=mu[i:i + 1])
        assert np.array_equal(m1[0], full[i][0]) and np.array_equal(v1[0], full[i][1]), (p, i)
    perms = [np.arange(70)[::-1], np.r_[np.arange(1, 70), 0], rng.permutation(70), np.r_[np.arange(0, 68), 69, 68]]
    for perm in perms:                                        # last items: on the longest series, the shortest, any
        rc, mean, var, off, sing, total = raw_kfilter(lib, ctx, which[perm], sig2[perm], roots[perm], ma[perm], mu[perm])
        assert rc == 0 and not sing.any()
        assert np.all(mean[total:] == -7.25) and np.all(var[total:] == -7.25), (p, perm[-1])
        for k, i in enumerate(perm):
            assert np.array_equal(mean[off[k]:off[k + 1]], full[i][0]) and np.array_equal(var[off[k]:off[k + 1]], full[i][1]), (p, i)


def test_car1_filter_items(lib):
    """k_mkfilter_car1: n in {2, 63, 64, 65, 129} x omega in {0.01, 0.3, 3}, 15 items in one call plus 70 more behind them (two
    waves), against oracle.kfilter_car1: 1e-9, scaled as in test_car1_filter_either_side_of_the_scan_switch."""
    series = []
    for n in (2, 63, 64, 65, 129):
        t, y, e = irregular_series(n, 600 + n)
        series.append((t, y + 5.0, e))
    ctx = lib.MultiContext(series, 1, 0)
    which = np.r_[np.repeat(np.arange(5), 3), np.arange(70) % 5]
    omega = np.r_[np.tile([0.01, 0.3, 3.0], 5), np.linspace(0.02, 2.0, 70)]
    mu = np.array([series[w][1].mean() for w in which])
    sig = np.array([2.0 * o * max(np.var(series[w][1]), 1.0) for o, w in zip(omega, which)])
    means, vars_, sing = ctx.kfilter(which, sig, -omega, None, mu=mu)
    assert not sing.any()
    for i in range(which.size):
        t, y, e = series[which[i]]
        yc = y - mu[i]
        om, ov = orc.kfilter_car1(t, yc, e, sig[i], omega[i])
        sc = max(np.abs(yc).max(), np.sqrt(ov[0]))
        assert means[i].shape == (t.size,), i
        assert np.max(np.abs(means[i] - mu[i] - om)) <= 1e-9 * sc, (i, which[i], omega[i])
        assert np.max(np.abs(vars_[i] - ov) / ov) <= 1e-9, (i, which[i], omega[i])
    # the first 15 alone, without mu on centred data: the same numbers to rounding of the shift
    ctx0 = lib.MultiContext([(t, y - y.mean(), e) for t, y, e in series], 1, 0)
    m0, v0, _ = ctx0.kfilter(which[:15], sig[:15], -omega[:15], None)
    for i in range(15):
        assert np.array_equal(v0[i], vars_[i]) and np.max(np.abs(m0[i] + mu[i] - means[i])) <= 1e-14 * 8.0, i


# ---------------------------------------------------------------------------------------------------------------------
# predict

def predict_times(t, rng, count):
    far_back, far_fore = t[0] - 5000.0, t[-1] + 5000.0
    k = min(7, t.size - 1)
    special = [far_back, t[0], t[k], 0.5 * (t[0] + t[1]), 0.5 * (t[-2] + t[-1]), far_fore, t[k], t[-1] + 1.5, t[0] - 2.5]
    more = rng.uniform(t[0] - 8.0, t[-1] + 8.0, max(count - len(special), 0))
    return rng.permutation(np.r_[special, more])[:count] if count < len(special) else rng.permutation(np.r_[special, more])


@pytest.mark.parametrize("p", range(1, 8))
def test_predict_items_at_every_order_and_group_edge(lib, p):
    """k_mpredict_carma<P,G> / k_mpredict_car1: items with 0, 1, E - 1, E, E + 1 and 3 E + 1 times (E = 64 / G pairs per wave; p =
    1: 64) on one series, one item each on a series of 2 and of 130 points, one series without items.  Far backcast, exactly
    t[0], an interior datum, midpoints, a repeated time and a far forecast, unsorted.  The bits of predict_carma /
    predict_car1 on the centred series alone (+ mu), the 50-digit conditional for the series of 40 and of 2 points, and the
    same bits when the n = 2 and n = 130 items share a call or not."""
    q = p - 1
    E = 64 if p == 1 else 64 // GROUP[p]
    rng = np.random.default_rng(9100 + p)
    series = []
    for k, n in enumerate((40, 2, 130, 25)):
        t, y, e = irregular_series(n, 930 + 10 * p + k)
        series.append((t, y + 3.0, e))
    ctx = lib.MultiContext(series, p, q)
    counts = (0, 1, E - 1, E, E + 1, 3 * E + 1)
    pool = predict_times(series[0][0], rng, 3 * E + 1)
    which = np.r_[np.zeros(6, dtype=int), 1, 2]
    times = [pool[:c] for c in counts] + [predict_times(series[1][0], rng, E + 1), predict_times(series[2][0], rng, E + 1)]
    M = which.size
    mu = np.array([series[w][1].mean() for w in which]) + rng.normal(0.0, 0.05, M)
    if p == 1:
        omega = np.array([0.04, 0.7, 0.04, 0.7, 0.04, 0.7, 0.3, 0.3])
        sig = np.array([2.0 * o * np.var(series[w][1]) for o, w in zip(omega, which)])
        roots, ma = -omega, None
        single = lambda i, tp: lib.predict_car1(series[which[i]][0], series[which[i]][1] - mu[i], series[which[i]][2], sig[i],  # noqa: E731
                                                omega[i], tp)
        truth = lambda i, tp: predict_truth_car1(series[which[i]][0], series[which[i]][1] - mu[i], series[which[i]][2], sig[i],  # noqa: E731
                                                 omega[i], tp)
        oracle = lambda i, tp: orc.predict_car1(series[which[i]][0], series[which[i]][1] - mu[i], series[which[i]][2], sig[i],  # noqa: E731
                                                omega[i], tp)
    else:
        kinds = ("complex", "mixed") if p > 2 else ("complex", "real")
        mods = [make_model(p, q, kinds[i % 2]) for i in range(M)]
        roots = np.array([m[0] for m in mods])
        ma = np.array([m[1] for m in mods])
        sig = np.array([np.var(series[w][1]) / m[2] for w, m in zip(which, mods)])
        single = lambda i, tp: lib.predict_carma(series[which[i]][0], series[which[i]][1] - mu[i], series[which[i]][2], sig[i],  # noqa: E731
                                                 roots[i], ma[i], tp)
        truth = lambda i, tp: predict_truth(series[which[i]][0], series[which[i]][1] - mu[i], series[which[i]][2], sig[i],  # noqa: E731
                                            roots[i], ma[i], tp)
        oracle = lambda i, tp: orc.predict_carma(series[which[i]][0], series[which[i]][1] - mu[i], series[which[i]][2], sig[i],  # noqa: E731
                                                 roots[i], ma[i], tp)
    pm, pv = ctx.predict(which, sig, roots, ma, times, mu=mu)
    assert [a.size for a in pm] == [t.size for t in times] and [a.size for a in pv] == [t.size for t in times]
    for i in range(M):
        if times[i].size == 0:
            continue
        sm, sv = single(i, times[i])
        assert np.array_equal(pm[i], sm + mu[i]) and np.array_equal(pv[i], sv), (p, i, times[i].size)
    # the exact conditional: items 4, 5 (models of both kinds, all the pool's times between them) and the n = 2 item
    for i in (4, 5, 6):
        tm, tv = truth(i, times[i])
        om, ov = oracle(i, times[i])
        assert_near_truth(pm[i] - mu[i], pv[i], tm, tv, om, ov, "set predict p=%d item %d" % (p, i))
    # n = 2 and n = 130 in one call, each alone, and the other way round
    sub = lambda idx: ctx.predict(which[idx], sig[idx], roots[idx], None if ma is None else ma[idx], [times[i] for i in idx],  # noqa: E731
                                  mu=mu[idx])
    for idx in ([6, 7], [7, 6], [6], [7]):
        a, b = sub(np.array(idx))
        for k, i in enumerate(idx):
            assert np.array_equal(a[k], pm[i]) and np.array_equal(b[k], pv[i]), (p, idx, i)


# ---------------------------------------------------------------------------------------------------------------------
# singular items, argument errors

def test_repeated_root_flags_its_item_only(lib):
    p = 4
    series = filter_set()[:8]
    ctx = lib.MultiContext(series, p, 1)
    _, roots, ma, sig2 = models_for(p, 1, 70, 7500)
    which = np.arange(70) % 8
    mu = np.full(70, 3.0)
    good_m, good_v, sing = ctx.kfilter(which, sig2, roots, ma, mu=mu)
    assert not sing.any()
    bad = roots.copy()
    bad[[3, 66]] = np.array(REPEATED_ROOTS[p], dtype=complex)
    m, v, sing = ctx.kfilter(which, sig2, bad, ma, mu=mu)
    assert np.array_equal(np.flatnonzero(sing), [3, 66])
    for i in range(70):
        if i not in (3, 66):
            assert np.array_equal(m[i], good_m[i]) and np.array_equal(v[i], good_v[i]), i
    times = [np.linspace(-5.0, 60.0, 1 + i % 5) for i in range(70)]
    gm, gv, sing = ctx.predict(which, sig2, roots, ma, times, mu=mu, return_singular=True)
    assert not sing.any()
    pm, pv, sing = ctx.predict(which, sig2, bad, ma, times, mu=mu, return_singular=True)
    assert np.array_equal(np.flatnonzero(sing), [3, 66])
    for i in range(70):
        if i not in (3, 66):
            assert np.array_equal(pm[i], gm[i]) and np.array_equal(pv[i], gv[i]), i
    with pytest.raises(lib.CarmaError):
        ctx.predict(which, sig2, bad, ma, times, mu=mu)


def test_argument_errors_leave_the_context_usable(lib):
    p = 3
    series = filter_set()[:6]
    ctx = lib.MultiContext(series, p, 2)
    _, roots, ma, sig2 = models_for(p, 2, 5, 7600)
    which = np.array([0, 5, 2, 2, 4])
    mu = np.full(5, 3.0)
    good = ctx.kfilter(which, sig2, roots, ma, mu=mu)

    def still_good():
        m, v, s = ctx.kfilter(which, sig2, roots, ma, mu=mu)
        assert all(np.array_equal(a, b) for a, b in zip(m, good[0])) and all(np.array_equal(a, b) for a, b in zip(v, good[1]))

    bad_which = which.copy()
    bad_which[3] = 6
    rc = raw_kfilter(lib, ctx, bad_which, sig2, roots, ma, mu)[0]
    assert rc == EINVAL and "item 3" in lib.last_error() and "out of range" in lib.last_error()
    still_good()
    bad_which[3] = -1
    assert raw_kfilter(lib, ctx, bad_which, sig2, roots, ma, mu)[0] == EINVAL and "item 3" in lib.last_error()
    open_roots = roots.copy()
    open_roots[2] = [-0.1 - 0.5j, -0.1 + 0.4j, -0.3]
    assert raw_kfilter(lib, ctx, which, sig2, open_roots, ma, mu)[0] == EINVAL and "item 2" in lib.last_error()
    with pytest.raises(ValueError):
        ctx.kfilter(which, sig2, open_roots, ma, mu=mu)
    still_good()
    for nma in (0, p + 1):
        assert raw_kfilter(lib, ctx, which, sig2, roots, ma, mu, nma=nma)[0] == EINVAL
    assert raw_kfilter(lib, ctx, which, sig2, roots, ma, mu, M=0)[0] == EINVAL
    assert raw_kfilter(lib, ctx, which, sig2, roots, ma, mu, M=-3)[0] == EINVAL
    still_good()
    # predict: a decreasing toff, named by its item
    om = np.ascontiguousarray(np.stack([roots.real, roots.imag], axis=-1))
    w32 = which.astype(np.int32)
    tp, pm, pv = np.linspace(0.0, 9.0, 10), np.zeros(10), np.zeros(10)
    toff = np.array([0, 4, 3, 6, 8, 10], dtype=np.int64)
    sig2, ma = np.ascontiguousarray(sig2), np.ascontiguousarray(ma)
    args = lambda to: (ctx.handle, w32.ctypes.data_as(_ip), 5, sig2.ctypes.data_as(_dp), om.ctypes.data_as(_dp),  # noqa: E731
                       ma.ctypes.data_as(_dp), ma.shape[1], mu.ctypes.data_as(_dp), tp.ctypes.data_as(_dp), to.ctypes.data_as(_lp),
                       pm.ctypes.data_as(_dp), pv.ctypes.data_as(_dp), None)
    assert lib.lib.carma_mpredict(*args(toff)) == EINVAL and "item 1" in lib.last_error()
    toff = np.array([0, 3, 3, 6, 8, 10], dtype=np.int64)       # item 1 has no times: legal
    assert lib.lib.carma_mpredict(*args(toff)) == 0
    want = ctx.predict(which, sig2, roots, ma, [tp[toff[i]:toff[i + 1]] for i in range(5)], mu=mu)
    assert np.array_equal(pm, np.concatenate(want[0])) and np.array_equal(pv, np.concatenate(want[1]))
    # the Python layer checks shapes before it calls
    with pytest.raises(ValueError):
        ctx.kfilter(which, sig2, roots[:4], ma, mu=mu)
    with pytest.raises(ValueError):
        ctx.kfilter(which, sig2, roots, ma[:, :0], mu=mu)
    with pytest.raises(ValueError):
        ctx.predict(which, sig2, roots, ma, [tp] * 4, mu=mu)
    with pytest.raises(ValueError):
        ctx.kfilter(bad_which, sig2, roots, ma, mu=mu)
    still_good()


# ---------------------------------------------------------------------------------------------------------------------
# CarmaModelSet

def test_model_set_assess_fit_and_predict(lib):
    """6 series with orders (1,0), (2,0), (3,2), (5,3) assigned through orders=, fits from get_mle: assess_fit and predict agree
    per series with KalmanFilterp / KalmanFilter1 built from the same mle_to_model model -- predictions bit equal, standardised
    residuals to 1e-9 of their scale (the one-model filter is the lane-group kernel) -- and resid_acf[0] == 1."""
    import carmcmc as cm
    orders = [(1, 0), (2, 0), (3, 2), (5, 3), (2, 0), (1, 0)]
    series = []
    for k, n in enumerate((40, 33, 64, 50, 21, 70)):
        t, y, e = irregular_series(n, 950 + k)
        series.append((t, y + 2.0, e))
    ms = cm.CarmaModelSet(series, p=2, q=0)
    rng = np.random.default_rng(951)
    fits = [None] * 6
    for (p, q) in sorted(set(orders)):
        if p == 1:
            starts = np.array([[[np.std(m.y), 1.0, m.y.mean(), np.log(rng.uniform(0.05, 0.5))] for _ in range(2)] for m in ms.models])
        else:
            starts = np.array([[prior_like_theta(rng, p, q, m.time, m.y) for _ in range(2)] for m in ms.models])
        res = ms.get_mle(p, q, starts=starts)
        for s, o in enumerate(orders):
            if o == (p, q):
                fits[s] = res[s]
    out = ms.assess_fit(fits, orders=orders, nplot=50)
    tgrid = np.r_[-30.0, np.linspace(0.0, 40.0, 9), 4000.0]
    pm_one, pv_one = ms.predict(tgrid, fits, orders=orders)
    pm_lst, pv_lst = ms.predict([tgrid[:s + 1] for s in range(6)], fits, orders=orders)
    for s, (m, (p, q)) in enumerate(zip(ms.models, orders)):
        sigsqr, roots, ma, mu = cm.mle_to_model(fits[s].x, p, q)
        tv, yv, ev = cm.vecD(m.time.tolist()), cm.vecD((m.y - mu).tolist()), cm.vecD(m.ysig.tolist())
        if p == 1:
            kf = cm.KalmanFilter1(tv, yv, ev, sigsqr, float(-roots[0].real))
        else:
            kf = cm.KalmanFilterp(tv, yv, ev, sigsqr, cm.vecC([complex(r) for r in roots]), cm.vecD(ma.tolist()))
        kf.Filter()
        kmean, kvar = np.array(kf.GetMean()), np.array(kf.GetVar())
        resid = (m.y - mu - kmean) / np.sqrt(kvar)
        d = out[s]
        assert d["std_resid"].shape == resid.shape and np.max(np.abs(d["std_resid"] - resid)) <= 1e-9 * np.abs(resid).max(), (s, p, q)
        assert d["resid_acf"][0] == 1.0 and d["resid_acf"].shape == resid.shape and np.all(np.abs(d["resid_acf"]) <= 1.0 + 1e-12)
        assert np.array_equal(d["time"], np.linspace(m.time.min(), m.time.max(), 50))
        a, b = kf.PredictBatch(d["time"])
        assert np.array_equal(d["mean"], np.asarray(a) + mu) and np.array_equal(d["var"], np.asarray(b)), (s, p, q)
        a, b = kf.PredictBatch(tgrid)
        assert np.array_equal(pm_one[s], np.asarray(a) + mu) and np.array_equal(pv_one[s], np.asarray(b)), (s, p, q)
        assert np.array_equal(pm_lst[s], pm_one[s][:s + 1]) and np.array_equal(pv_lst[s], pv_one[s][:s + 1]), (s, p, q)


@pytest.mark.parametrize("p,q", REGROW_ORDERS)
def test_one_context_regrows_its_item_buffers(lib, p, q):
    """One MultiContext on series of 20, 33 and 70 points: kfilter of 2, 130 and 2 items (130: three waves, and at p = 5 a
    parameter upload of 130 x 17 doubles, past the 4096-byte floor of the grown buffers), then predict at 3 times in all, at 700
    spread unevenly with one item given none, and at 3 again.  Every result equals that of a fresh context making only that call."""
    series = regrow_series()
    sig, roots, ma = regrow_models(p, q, 130, 60 + 10 * p + q)
    if p == 1:
        roots = roots[:, 0]
    which = np.arange(130) % 3
    ctx = lib.MultiContext(series, p, q)
    for step, M in enumerate((2, 130, 2)):
        fresh = lib.MultiContext(series, p, q)
        call = (which[:M], sig[:M], roots[:M], ma[:M])
        got, want = ctx.kfilter(*call, mu=sig[:M] - 1.0), fresh.kfilter(*call, mu=sig[:M] - 1.0)
        fresh.close()
        assert not want[2].any() and all(np.isfinite(a).all() for a in want[0] + want[1])
        assert_all_equal(got, want, "kfilter CARMA(%d,%d) step %d" % (p, q, step))
    rng = np.random.default_rng(8)
    item = (np.array([2, 0, 1, 2]), sig[:4], roots[:4], ma[:4])
    for step, counts in enumerate(((2, 0, 1, 0), (300, 0, 250, 150), (2, 0, 1, 0))):
        times = [rng.uniform(-5.0, 150.0, k) for k in counts]
        fresh = lib.MultiContext(series, p, q)
        got, want = ctx.predict(*item, times), fresh.predict(*item, times)
        fresh.close()
        assert all(np.isfinite(a).all() for a in want[0] + want[1])
        assert_all_equal(got, want, "predict CARMA(%d,%d) step %d" % (p, q, step))
    ctx.close()
