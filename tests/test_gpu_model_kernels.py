"""The filter, predict and simulate kernels behind the reference API -- KalmanFilterp / KalmanFilter1 (Filter, Predict,
PredictBatch, Simulate), CarmaSample.predict / assess_fit / simulate, carma_process(_batch), car1_process(_batch) -- at every
order p = 2..7 and at the launch edges where lane-group kernels go wrong: item counts on either side of a wave (64 / G items
per wave, G = 2, 4 or 8 lanes per model; the groups past the last item redo it and must store nothing new), series of one or
two points, repeated and unsorted times, one handle whose device buffer grows and shrinks between calls.

Yardsticks: predict -- the dense Gaussian-process conditional at 50 digits (mp_truth.predict_truth), the oracle only as the
arbiter's other side; simulate -- the construction itself: filtering a path with yerr = 0 gives back the counter-based normal
draws it was built from; filter -- the one-model entry point and the oracle, with the quad-precision filter as arbiter."""
import numpy as np
import pytest

import oracle as orc
from helpers import (ROOT_KINDS, irregular_series, model_ma, model_roots, philox_normals, prior_like_theta,
                     record_allowance)
from mp_truth import predict_truth, predict_truth_car1

pytestmark = pytest.mark.gpu

GROUP = {2: 2, 3: 4, 4: 4, 5: 8, 6: 8, 7: 8}          # lanes per model: GroupOf<P> (carma_kernels.hip)
MODELS = [(p, q, kind) for p in range(2, 8) for q in (0, p - 1) for kind in (ROOT_KINDS if p > 2 else ROOT_KINDS[:2])]
MODEL_IDS = ["p%dq%d-%s" % m for m in MODELS]


@pytest.fixture(scope="module")
def lib():
    from carma_pack_amd import _lib
    assert _lib.lib.carma_device_count() >= 1
    return _lib


def counts(G, last):
    """1, a wave short by one, a full wave, one into the next wave, and `last` (several waves, shadow groups at the end)."""
    E = 64 // G
    return (1, E - 1, E, E + 1, last)


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
    """irregular_series, centred, with the process variance (sigsqr = var(y) / variance at sigsqr 1) matched to the data."""
    t, y, yerr = irregular_series(n, seed)
    y = y - y.mean()
    return t, y, yerr, float(np.var(y) / v1)


def assert_near_truth(got_m, got_v, tm, tv, om, ov, what, rtol=1e-9):
    """Predictions against the exact (50-digit) values: variances to rtol relative, means to rtol of max(|mean|, sd).  An entry
    beyond rtol passes only where the oracle misses rtol as well and the device is no further from the exact value than the
    oracle is (the assert_parity arbiter rule); every such entry is counted."""
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
    if nb:
        record_allowance("predict: device beyond %.0e of the 50-digit value, no further than the oracle" % rtol, what, nb, nb,
                         2 * got_m.size)


# ---------------------------------------------------------------------------------------------------------------------
# predict

@pytest.mark.parametrize("p,q,kind", MODELS, ids=MODEL_IDS)
def test_predict_at_every_order_and_launch_edge(lib, p, q, kind):
    """k_predict_carma<P,G>: backcasts far and near, exactly t[0] and interior data times, midpoints, repeated and unsorted
    times, forecasts near and far, for M on both sides of a wave and several waves with shadow groups."""
    import carma_pack_amd as cpa
    roots, ma, v1 = make_model(p, q, kind)
    t, y, yerr, sigsqr = centred_series(48, 70 + 10 * p + q, v1)
    G = GROUP[p]
    Mmax = 3 * (64 // G) + 1
    rng = np.random.default_rng(900 + 10 * p + q)
    far_back, far_fore = t[0] - 5000.0, t[-1] + 5000.0
    special = [far_back, t[0] - 2.5, t[0], t[1], t[7], t[24], t[-1], 0.5 * (t[3] + t[4]), 0.5 * (t[-2] + t[-1]),
               t[-1] + 1.5, far_fore]
    special += [special[4], special[7]]                                   # repeated prediction times
    tp = rng.permutation(np.r_[special, rng.uniform(t[0] - 8.0, t[-1] + 8.0, Mmax - len(special))])   # unsorted
    tm, tv = predict_truth(t, y, yerr, sigsqr, roots, ma, tp)
    om, ov = orc.predict_carma(t, y, yerr, sigsqr, roots, ma, tp)
    what = "predict p=%d q=%d %s" % (p, q, kind)
    for M in counts(G, Mmax):
        pm, pv = lib.predict_carma(t, y, yerr, sigsqr, roots, ma, tp[:M])
        assert_near_truth(pm, pv, tm[:M], tv[:M], om[:M], ov[:M], "%s M=%d" % (what, M))
    # (pm, pv: all Mmax times) the far forecast and backcast forget the data: the stationary moments
    v0 = cpa.carma_variance(sigsqr, roots, ma)
    for far in (far_back, far_fore):
        i = int(np.flatnonzero(tp == far)[0])
        assert abs(pm[i]) <= 1e-12 * np.sqrt(v0), (what, far, pm[i])
        assert abs(pv[i] - v0) <= 1e-9 * v0, (what, far, pv[i], v0)
    # a repeated time gives the same bits wherever it sits in the launch
    for x in (special[4], special[7]):
        i = np.flatnonzero(tp == x)
        assert i.size >= 2 and np.all(pm[i] == pm[i[0]]) and np.all(pv[i] == pv[i[0]]), (what, x)


@pytest.mark.parametrize("p", range(2, 8))
def test_predict_on_series_edges(lib, p):
    """n = 1, n = 2, a series whose times all collapse to one after sort_dedup, and an unsorted series with duplicated times:
    the same bits as the call on oracle.sort_dedup of the input, and the exact values of the deduplicated series."""
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
        pm, pv = lib.predict_carma(tt, yy, ee, sigsqr, roots, ma, tp)
        pm2, pv2 = lib.predict_carma(ts, ys, es, sigsqr, roots, ma, tp)
        assert np.array_equal(pm, pm2) and np.array_equal(pv, pv2), (p, name)
        tm, tv = predict_truth(ts, ys, es, sigsqr, roots, ma, tp)
        om, ov = orc.predict_carma(ts, ys, es, sigsqr, roots, ma, tp)
        assert_near_truth(pm, pv, tm, tv, om, ov, "predict p=%d %s" % (p, name))


def test_predict_car1_at_lane_counts(lib):
    """k_predict_car1 (one lane per time) at M = 1, 63, 64, 65, 200 against the 50-digit CAR(1) conditional."""
    t, y, yerr = irregular_series(60, 31)
    y = y - y.mean()
    rng = np.random.default_rng(32)
    for omega in (0.04, 0.7):
        sigsqr = 2.0 * omega * np.var(y)
        tp = rng.permutation(np.r_[t[0] - 4000.0, t[0] - 3.0, t[0], t[5], t[-1], 0.5 * (t[8] + t[9]), t[-1] + 2.0,
                                   t[5], t[-1] + 4000.0, rng.uniform(t[0] - 5.0, t[-1] + 5.0, 191)])
        tm, tv = predict_truth_car1(t, y, yerr, sigsqr, omega, tp)
        om, ov = orc.predict_car1(t, y, yerr, sigsqr, omega, tp)
        for M in (1, 63, 64, 65, 200):
            pm, pv = lib.predict_car1(t, y, yerr, sigsqr, omega, tp[:M])
            assert_near_truth(pm, pv, tm[:M], tv[:M], om[:M], ov[:M], "predict car1 omega=%g M=%d" % (omega, M))


REPEATED_ROOTS = {2: [-0.2, -0.2], 4: [-0.1 - 0.5j, -0.1 + 0.5j, -0.1 - 0.5j, -0.1 + 0.5j],
                  7: [-0.1 - 0.5j, -0.1 + 0.5j, -0.3, -0.3, -0.5, -0.8, -1.2]}


@pytest.mark.parametrize("p", sorted(REPEATED_ROOTS))
def test_repeated_ar_root_is_an_error(lib, p):
    """A repeated AR root makes the eigenvector matrix singular (the reference's solve throws, kfilter.cpp:157-158):
    CarmaError from filter, predict and simulate, never numbers."""
    roots = np.array(REPEATED_ROOTS[p], dtype=complex)
    ma = np.r_[1.0, np.zeros(p - 1)]
    t, y, yerr = irregular_series(20, 5)
    with pytest.raises(lib.CarmaError):
        lib.kfilter_carma(t, y, yerr, 1.0, roots, ma)
    with pytest.raises(lib.CarmaError):
        lib.predict_carma(t, y, yerr, 1.0, roots, ma, np.linspace(t[0], t[-1], 40))
    with pytest.raises(lib.CarmaError):
        lib.simulate_carma(t, 1.0, roots, ma, npaths=40, seed=3)


@pytest.mark.parametrize("p", (1, 3, 6))
def test_kalman_handle_reused_while_its_device_memory_grows_and_shrinks(lib, p):
    """One KalmanFilterp / KalmanFilter1 handle driven through Filter -> PredictBatch(300) -> PredictBatch(5) -> Filter ->
    PredictBatch(301) -> Predict(x): its device buffer holds 2n doubles for Filter and 3M for Predict, grows and is reused;
    every result is bitwise the one-shot entry point's."""
    import carmcmc as cm
    t, y, yerr = irregular_series(150, 80 + p)
    y = y - y.mean()
    rng = np.random.default_rng(81 + p)
    tps = [rng.uniform(t[0] - 10.0, t[-1] + 10.0, M) for M in (300, 5, 301)]
    x = float(0.5 * (t[40] + t[41]))
    tv, yv, ev = cm.vecD(t.tolist()), cm.vecD(y.tolist()), cm.vecD(yerr.tolist())
    if p == 1:
        sigsqr, omega = 0.3, 0.05
        kf = cm.KalmanFilter1(tv, yv, ev, sigsqr, omega)
        filt = lambda: lib.kfilter_car1(t, y, yerr, sigsqr, omega)                      # noqa: E731
        pred = lambda s: lib.predict_car1(t, y, yerr, sigsqr, omega, s)                  # noqa: E731
    else:
        roots, ma, v1 = make_model(p, 1, "mixed")
        sigsqr = float(np.var(y) / v1)
        kf = cm.KalmanFilterp(tv, yv, ev, sigsqr, cm.vecC([complex(r) for r in roots]), cm.vecD(ma.tolist()))
        filt = lambda: lib.kfilter_carma(t, y, yerr, sigsqr, roots, ma)                 # noqa: E731
        pred = lambda s: lib.predict_carma(t, y, yerr, sigsqr, roots, ma, s)             # noqa: E731
    m1, v1_ = filt()

    def filter_matches():
        kf.Filter()
        assert np.array_equal(np.array(kf.GetMean()), m1) and np.array_equal(np.array(kf.GetVar()), v1_), p

    def batch_matches(s):
        a, b = kf.PredictBatch(s)
        wa, wb = pred(s)
        assert np.array_equal(a, wa) and np.array_equal(b, wb), (p, s.size)

    filter_matches()
    batch_matches(tps[0])
    batch_matches(tps[1])
    filter_matches()
    batch_matches(tps[2])
    pr = kf.Predict(x)
    wa, wb = pred(np.array([x]))
    assert pr.first == wa[0] and pr.second == wb[0]


# ---------------------------------------------------------------------------------------------------------------------
# simulate

def whitened(path, t, sigsqr, roots, ma):
    """The standardised innovations of a noise-free path under its own model (the oracle's filter with yerr = 0): exactly
    the normal draws the path was built from."""
    mean, var = orc.kfilter_carma(t, path, np.zeros(t.size), sigsqr, roots, ma)
    return (path - mean) / np.sqrt(var)


@pytest.mark.parametrize("p,q,kind", MODELS, ids=MODEL_IDS)
def test_simulate_is_the_exact_construction_at_every_order(lib, p, q, kind):
    """k_simulate_carma<P,G>: for every launch size around a wave, the first path, the last, and the last live path of every
    wave give back their Philox normals when filtered with yerr = 0; path k has the same bits whatever the launch size."""
    roots, ma, v1 = make_model(p, q, kind)
    t = irregular_series(40, 20 + p)[0]
    sigsqr = 1.0 / v1
    G = GROUP[p]
    E = 64 // G
    N = 5 * E + 3
    seed = 0x5EED0000 + 1000 * p + 10 * q + ROOT_KINDS.index(kind)
    big = lib.simulate_carma(t, sigsqr, roots, ma, npaths=N, seed=seed)
    assert big.shape == (N, t.size) and np.all(np.isfinite(big))
    check = set()
    for n in counts(G, N):
        got = lib.simulate_carma(t, sigsqr, roots, ma, npaths=n, seed=seed)
        assert np.array_equal(got, big[:n]), (p, q, kind, n)
        check |= {0, n - 1} | {min((w + 1) * E, n) - 1 for w in range((n + E - 1) // E)}
    for k in sorted(check):
        np.testing.assert_allclose(whitened(big[k], t, sigsqr, roots, ma), philox_normals(seed, k, t.size), rtol=0, atol=2e-7,
                                   err_msg="p=%d q=%d %s path %d" % (p, q, kind, k))


@pytest.mark.parametrize("p", (2, 4, 7))
def test_simulate_key_uses_the_high_seed_bits(lib, p):
    """Seeds that differ only above bit 32 draw different paths, each its own restatement's."""
    roots, ma, v1 = make_model(p, p - 1, "complex")
    t = irregular_series(30, 7)[0]
    lo = 0x89ABCDEF
    paths = {}
    for seed in (lo, lo | (1 << 32), lo | (0x7F3 << 44)):
        paths[seed] = lib.simulate_carma(t, 1.0 / v1, roots, ma, npaths=3, seed=seed)
        for k in range(3):
            np.testing.assert_allclose(whitened(paths[seed][k], t, 1.0 / v1, roots, ma), philox_normals(seed, k, t.size),
                                       rtol=0, atol=2e-7)
    s = sorted(paths)
    for i in range(3):
        for j in range(i + 1, 3):
            assert not np.any(paths[s[i]] == paths[s[j]]), (p, hex(s[i]), hex(s[j]))


def test_car1_paths_are_the_ou_recursion(lib):
    """k_simulate_car1 (one lane per path): every path of every launch size around a wave is the Ornstein-Uhlenbeck
    recursion (car1_process) restated with the Philox normals: rtol 1e-12 (atol 1e-12 of the process scale, for values
    that pass near zero), and the same bits whatever the launch size."""
    t = irregular_series(50, 12)[0]
    for (sigsqr, omega, seed) in ((0.5, 0.05, 5 | (3 << 40)), (2.0, 1.3, 0xFEEDFACE12)):
        sv = sigsqr / (2.0 * omega)
        N = 5 * 64 + 3
        big = lib.simulate_car1(t, sigsqr, omega, npaths=N, seed=seed)
        for n in (1, 63, 64, 65, N):
            assert np.array_equal(lib.simulate_car1(t, sigsqr, omega, npaths=n, seed=seed), big[:n]), n
        rho = np.exp(-np.diff(t) * omega)
        for k in range(N):
            z = philox_normals(seed, k, t.size)
            want = np.empty(t.size)
            want[0] = np.sqrt(sv) * z[0]
            for i in range(1, t.size):
                want[i] = rho[i - 1] * want[i - 1] + np.sqrt(sv * (1.0 - rho[i - 1] ** 2)) * z[i]
            np.testing.assert_allclose(big[k], want, rtol=1e-12, atol=1e-12 * np.sqrt(sv), err_msg="path %d" % k)


def exact_process_with_repeats(time, sigsqr, roots, ma, z):
    """carma_pack.carma_process (the D = P - V form of the reference's construction, carma_pack.py:1148-1259) fed the normals
    z[i] in place of np.random.normal, with the exact limit at a repeated time: the one-step variance there is exactly 0, so
    the value repeats and the next step makes no measurement update; the path goes on with z[i] of its sorted position i.
    (The reference itself computes that variance at rounding size: negative, np.sqrt gives NaN and np.random.normal(mean, nan)
    returns NaN for the value -- NumPy 2.2 raises nothing -- and the rest of the path is NaN; positive, the update divides by
    it and every later value is off by ~sqrt(eps) of the path's scale.)"""
    from carma_pack_amd import carma_pack as cp
    r = np.asarray(roots, dtype=complex)
    b, V = cp._rotated_system(sigsqr, r, ma)
    c = V @ np.conj(b)
    s0 = float(np.real(b @ c))
    D = np.zeros((r.size, r.size), dtype=complex)
    x = np.zeros(r.size, dtype=complex)
    y = np.empty(time.size)
    var, mean = s0, 0.0
    y[0] = np.sqrt(var) * z[0]
    innov, u = y[0], c.copy()
    for k in range(1, time.size):
        rho = np.exp(r * (time[k] - time[k - 1]))
        if var > 0.0:
            x = x + u * (innov / var)
            D = D - np.outer(u, np.conj(u)) / var
        x, D = rho * x, np.outer(rho, np.conj(rho)) * D
        w = D @ np.conj(b)
        u = w + c
        mean = float(np.real(b @ x))
        if time[k] == time[k - 1]:
            var, y[k] = 0.0, y[k - 1]
        else:
            var = s0 + float(np.real(b @ w))
            y[k] = mean + np.sqrt(var) * z[k]
        innov = y[k] - mean
    return y


@pytest.mark.parametrize("p", (2, 3, 5, 7))
def test_simulate_through_repeated_times(lib, p):
    """Unsorted times with repeats (a pair at the start, a triple inside, a pair at the end): each path is the exact
    construction's limit to 1e-8 of the process scale -- the value repeats, the state does not move -- and the host's
    carma_process, fed the same normals, is the same limit."""
    from carma_pack_amd import carma_pack as cp
    kind = "complex" if p % 2 == 0 else "mixed"
    roots, ma, v1 = make_model(p, p - 1, kind)
    sigsqr = 1.0 / v1
    t0 = irregular_series(30, 50 + p)[0]
    rng = np.random.default_rng(p)
    series = {"pair, triple, pair": np.r_[t0, t0[0], t0[12], t0[12], t0[-1]],
              "one repeat": np.r_[t0, t0[5]]}
    for name, tt in series.items():
        tt = rng.permutation(tt)
        ts = np.sort(tt)
        paths = lib.simulate_carma(tt, sigsqr, roots, ma, npaths=3, seed=11)
        for k in range(3):
            z = philox_normals(11, k, ts.size)
            want = exact_process_with_repeats(ts, sigsqr, roots, ma, z)
            err = np.max(np.abs(paths[k] - want))
            assert err <= 1e-8, "p=%d %s path %d: %.3e from the exact limit (process sd 1)" % (p, name, k, err)

            class Feed(object):                                           # rng.normal(mean, sd) -> mean + sd z[i]
                i = 0

                def normal(self, m, sd):
                    self.i += 1
                    return m + sd * z[self.i - 1]

            host = cp.carma_process(tt, sigsqr, roots, ma, rng=Feed())
            assert np.max(np.abs(host - want)) <= 1e-8, (p, name, k)


# ---------------------------------------------------------------------------------------------------------------------
# filter

@pytest.mark.parametrize("p", (2, 4, 6))
def test_batched_filter_at_tile_edges(lib, p):
    """k_kfilter_carma_lane + k_transpose_mv (32 x 32 tiles, ld = B + 64) over B in {1, 31, 32, 33, 63, 64, 65, 130} x n in
    {2, 31, 32, 33, 65}: every element of every model against the one-model entry point and the oracle -- variances to 1e-9
    relative, means to 1e-9 of the data's scale, or no further from the quad-precision filter than 1.25 x the oracle (the
    rule of test_gpu_parity.test_filter_of_many_models_in_one_launch) -- and model b's rows the same bits in every batch."""
    q = p // 2
    rng = np.random.default_rng(7000 + p)
    t0, y0, _ = irregular_series(65, 300 + p)
    th = np.array([prior_like_theta(rng, p, q, t0, y0) for _ in range(130)])
    roots = np.array([orc.ar_roots(x, p) for x in th])
    ma = np.array([orc.ma_coefs(x, p, q) for x in th])[:, : q + 1]
    sig2 = np.array([x[0] ** 2 / orc.variance(r, m) for x, r, m in zip(th, roots, ma)])
    nworse, ntot = 0, 0
    for n in (2, 31, 32, 33, 65):
        t, y, yerr = irregular_series(n, 400 + 10 * p + n)
        y = y - y.mean()
        one = [lib.kfilter_carma(t, y, yerr, sig2[i], roots[i], ma[i]) for i in range(130)]
        orac = [orc.kfilter_carma(t, y, yerr, sig2[i], roots[i], ma[i]) for i in range(130)]
        sc = np.abs(y).max()
        full = None
        for B in (130, 1, 31, 32, 33, 63, 64, 65):
            mean, var, sing = lib.kfilter_carma_batch(t, y, yerr, sig2[:B], roots[:B], ma[:B])
            assert mean.shape == (B, n) and var.shape == (B, n) and not sing.any(), (p, n, B)
            if full is None:
                full = (mean, var)
            else:
                assert np.array_equal(mean, full[0][:B]) and np.array_equal(var, full[1][:B]), (p, n, B)
        mean, var = full
        for i in range(130):
            (m1, v1), (om, ov) = one[i], orac[i]
            d_dev = max(np.max(np.abs(mean[i] - om)) / sc, np.max(np.abs(var[i] - ov) / ov))
            d_one = max(np.max(np.abs(m1 - om)) / sc, np.max(np.abs(v1 - ov) / ov))
            d_pair = max(np.max(np.abs(mean[i] - m1)) / sc, np.max(np.abs(var[i] - v1) / v1))
            ntot += 1
            if max(d_dev, d_one, d_pair) > 1e-9:
                thx = th[i].copy()
                thx[1], thx[2] = 1.0, 0.0
                tm, tv = orc.truth_filter(t, y, yerr, thx, p, q)
                eo = max(np.max(np.abs(om - tm)) / sc, np.max(np.abs(ov - tv) / tv))
                for got_m, got_v, who in ((mean[i], var[i], "batched"), (m1, v1, "one-model")):
                    eg = max(np.max(np.abs(got_m - tm)) / sc, np.max(np.abs(got_v - tv) / tv))
                    assert eg <= max(1e-9, 1.25 * eo), (p, n, i, who, eg, eo)
                nworse += 1
    assert nworse <= 0.1 * ntot, (nworse, ntot)
    if nworse:
        record_allowance("batched filter: beyond 1e-9, no further from the quad-precision filter than 1.25 x the oracle",
                         "p=%d" % p, nworse, int(0.1 * ntot), ntot)
    # n = 1 has no batched form: a clean error, not numbers
    with pytest.raises((ValueError, lib.CarmaError)):
        lib.kfilter_carma_batch(t[:1], y[:1], yerr[:1], sig2[:3], roots[:3], ma[:3])


@pytest.mark.parametrize("p", range(2, 8))
def test_single_model_filter_short_and_odd_lengths(lib, p):
    """k_kfilter_carma<P,G> (one model, one wave) at n = 1, 2, 3, 33, 65 against the oracle: 1e-9."""
    roots, ma, v1 = make_model(p, p - 1, "mixed" if p > 2 else "complex")
    for n in (1, 2, 3, 33, 65):
        t, y, yerr, sigsqr = centred_series(n, 500 + 10 * p + n, v1) if n > 1 else (np.array([3.0]), np.array([0.7]),
                                                                                      np.array([0.4]), 1.0 / v1)
        m, v = lib.kfilter_carma(t, y, yerr, sigsqr, roots, ma)
        om, ov = orc.kfilter_carma(t, y, yerr, sigsqr, roots, ma)
        assert m.shape == (n,) and v.shape == (n,)
        sc = max(np.abs(y).max(), np.sqrt(ov[0]))
        assert np.max(np.abs(m - om)) <= 1e-9 * sc and np.max(np.abs(v - ov) / ov) <= 1e-9, (p, n)


def test_car1_filter_either_side_of_the_scan_switch(lib):
    """KalmanFilter1::Filter: k_kfilter_car1 (one lane) below n = 64, k_kfilter_car1_scan (the series across a wave) from 64
    on; n = 1, 2, 63, 64, 65, 127, 128, 129 against oracle.kfilter_car1: 1e-9."""
    for n in (1, 2, 63, 64, 65, 127, 128, 129):
        t, y, yerr = irregular_series(n, 600 + n)
        y = y - y.mean()
        for omega in (0.01, 0.3, 3.0):
            sigsqr = 2.0 * omega * max(np.var(y), 1.0)
            m, v = lib.kfilter_car1(t, y, yerr, sigsqr, omega)
            om, ov = orc.kfilter_car1(t, y, yerr, sigsqr, omega)
            sc = max(np.abs(y).max(), np.sqrt(ov[0]))
            assert m.shape == (n,) and np.max(np.abs(m - om)) <= 1e-9 * sc, (n, omega)
            assert np.max(np.abs(v - ov) / ov) <= 1e-9, (n, omega)
