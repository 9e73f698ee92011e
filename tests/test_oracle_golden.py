"""Pins the CPU oracle (oracle/carma_oracle.c) against the golden vectors generated from the
reference's own Python (tests/golden/make_golden.py) and against the reference's known answers.
No GPU needed."""
import json
import os

import numpy as np
import pytest

import oracle as orc

RTOL_LL = 1e-12   # SURVEY §7 stage 1 bar for the restatement
RTOL_ILL = 1e-11  # cases with cond(E) > 1e5


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def _check_case(t, y, yerr, th, p, q, g_omega, g_ma, g_sig, g_mean, g_var, g_ll, cond):
    """Restatement vs reference Python (scipy/LAPACK LU): the two LU's differ at rounding level, so
    per-element bars are loose where the Vandermonde system is ill-conditioned; the log-likelihood
    bar is the tight one (1e-11 always, 1e-12 on well-conditioned cases)."""
    om = orc.ar_roots(th, p)
    ma = orc.ma_coefs(th, p, q)
    np.testing.assert_allclose(om, g_omega, rtol=1e-13, atol=0)
    np.testing.assert_allclose(ma, g_ma, rtol=1e-12, atol=1e-15)
    sig = th[0] ** 2 / orc.variance(om, ma)
    assert abs(sig - g_sig) <= 1e-11 * abs(g_sig)
    mean, var = orc.kfilter_carma(t, y - th[2], np.sqrt(th[1]) * yerr, sig, om, ma)
    np.testing.assert_allclose(var, g_var, rtol=1e-8)
    np.testing.assert_allclose(mean, g_mean, rtol=0, atol=1e-10 * np.abs(y - th[2]).max())
    m = orc.OracleModel(t, y, yerr, p, q)
    ll = m.logdensity(th, ignore_prior=True) - m.log_prior(th)
    tol = RTOL_ILL if cond > 1e3 else RTOL_LL
    assert abs(ll - g_ll) <= tol * abs(g_ll)
    return abs(ll - g_ll) / abs(g_ll)


def test_readme_carma53_matches_reference_python(golden_dir):
    g = _load(golden_dir, "carma53_readme.npz")
    t, y, yerr, p, q = g["t"], g["y"], g["yerr"], int(g["p"]), int(g["q"])
    assert t.size == 270 and (p, q) == (5, 3)
    for i in range(g["theta"].shape[0]):
        _check_case(t, y, yerr, g["theta"][i], p, q, g["omega"][i], g["ma"][i], g["sigsqr"][i],
                    g["mean"][i], g["var"][i], g["loglik"][i], g["cond"][i])


def test_readme_dense_gp_identity(golden_dir):
    """carma_unit_tests.cpp:564-594: Kalman log-lik == dense GP log-lik."""
    g = _load(golden_dir, "carma53_readme.npz")
    m = orc.OracleModel(g["t"], g["y"], g["yerr"], 5, 3)
    idx = np.flatnonzero(np.isfinite(g["dense_loglik"]))
    assert idx.size >= 4
    for i in idx:
        th = g["theta"][i]
        ll = m.logdensity(th, ignore_prior=True) - m.log_prior(th)
        assert abs(ll - g["dense_loglik"][i]) <= 1e-9 * abs(ll)


def test_readme_true_model_filter(golden_dir):
    g = _load(golden_dir, "carma53_readme.npz")
    mean, var = orc.kfilter_carma(g["t"], g["y"] - 17.0, g["yerr"], float(g["true_sigsqr"]), g["true_omega"],
                                  g["true_ma"])
    np.testing.assert_allclose(var, g["true_var"], rtol=1e-12)
    np.testing.assert_allclose(mean, g["true_mean"], rtol=0, atol=1e-12)
    # var(0) identity (carma_unit_tests.cpp:443-444): var0 = sigma_y^2 + yerr0^2, sigma_y = 2.3
    assert abs(var[0] - (2.3 ** 2 + g["yerr"][0] ** 2)) < 1e-10


def test_car1_matches_dense_gp(golden_dir):
    g = _load(golden_dir, "car1_n100.npz")
    t, y, yerr = g["t"], g["y"], g["yerr"]
    m = orc.OracleModel(t, y, yerr, 1)
    for i in range(g["theta"].shape[0]):
        th = g["theta"][i]
        omega = np.exp(th[3])
        mean, var = orc.kfilter_car1(t, y - th[2], np.sqrt(th[1]) * yerr, 2 * th[0] ** 2 * omega, omega)
        np.testing.assert_allclose(var, g["var"][i], rtol=1e-9)
        np.testing.assert_allclose(mean, g["mean"][i], rtol=0, atol=1e-9)
        # var(0) identity (carma_unit_tests.cpp:215-216)
        assert abs(var[0] - (th[0] ** 2 + th[1] * yerr[0] ** 2)) < 1e-10
        # logdensity - prior == dense GP loglik; the CAR1 bounds have no ignore_prior switch
        if m.check_prior_bounds(th):
            ll = m.logdensity(th) - m.log_prior(th)
            assert abs(ll - g["dense_loglik"][i]) <= 1e-9 * abs(ll)


def test_ogle_grid(golden_dir):
    g = _load(golden_dir, "ogle_grid.npz")
    t, y, yerr = g["t"], g["y"], g["yerr"]
    assert t.size == 437
    n_checked = 0
    for p in range(2, 8):
        for q in range(p):
            k = "p%dq%d_" % (p, q)
            for i in range(g[k + "theta"].shape[0]):
                cond = g[k + "cond"][i]
                _check_case(t, y, yerr, g[k + "theta"][i], p, q, g[k + "omega"][i], g[k + "ma"][i],
                            g[k + "sigsqr"][i], g[k + "mean"][i], g[k + "var"][i], g[k + "loglik"][i], cond)
                n_checked += 1
    assert n_checked == 81


def test_cpp_fixture_filter(golden_dir):
    """First 300 rows of cpp_tests/data/carma_test.dat with the true ZCARMA(5) parameters of
    carma_unit_tests.cpp:387-503."""
    g = _load(golden_dir, "cpp_carma_test300.npz")
    mean, var = orc.kfilter_carma(g["t"], g["y"], g["yerr"], float(g["sigsqr"]), g["omega"], g["ma"])
    np.testing.assert_allclose(var, g["var"], rtol=1e-11)
    np.testing.assert_allclose(mean, g["mean"], rtol=0, atol=1e-11)
    assert abs(var[0] - (2.3 ** 2 + g["yerr"][0] ** 2)) < 1e-10


def test_variance_known_answer(golden_dir):
    """carma_unit_tests.cpp:1269-1317: Variance(...) = 223003.230567 to rel 1e-8."""
    s = json.load(open(os.path.join(golden_dir, "summary.json")))["variance_kat"]
    om = np.array(s["omega_re"]) + 1j * np.array(s["omega_im"])
    v = orc.variance(om, s["ma"], sigma=2.3)
    assert abs(v - s["expected_cpp"]) / s["expected_cpp"] < 1e-8
    assert abs(v - s["python"]) / s["python"] < 1e-13
    for lag, ref in zip(s["lags"], s["lagged"]):
        assert abs(orc.variance(om, s["ma"], sigma=2.3, dt=lag) - ref) / abs(ref) < 1e-12


def test_sort_and_dedup():
    """carma_unit_tests.cpp:55-187: n=100 linspace, swap idx 12<->43, duplicate idx 43."""
    t = np.linspace(0.0, 99.0, 100)
    y = np.arange(100.0) * 2
    e = np.arange(100.0) + 0.5
    t2, y2, e2 = t.copy(), y.copy(), e.copy()
    for a in (t2, y2, e2):
        a[[12, 43]] = a[[43, 12]]
    ts, ys, es = orc.sort_dedup(t2, y2, e2)
    np.testing.assert_array_equal(ts, t)
    np.testing.assert_array_equal(ys, y)
    np.testing.assert_array_equal(es, e)
    t3 = np.insert(t, 43, t[43])
    y3 = np.insert(y, 43, -1.0)
    e3 = np.insert(e, 43, -1.0)
    ts, ys, es = orc.sort_dedup(t3, y3, e3)
    assert ts.size == 100 and np.all(np.diff(ts) > 0)
    # the FIRST of the duplicated pair is kept (unique_values = {0} U 1+find(dt != 0))
    assert ys[43] == -1.0 and ys[44] == y[44]


def test_prior_bounds(golden_dir):
    """carma_unit_tests.cpp:1116-1267 + carpack.cpp:314-374."""
    g = _load(golden_dir, "carma53_readme.npz")
    m = orc.OracleModel(g["t"], g["y"], g["yerr"], 5, 3)
    th = g["theta"][0].copy()
    assert np.isfinite(m.logdensity(th))

    def bad(mod):
        x = th.copy()
        mod(x)
        assert m.logdensity(x) == -np.inf
        assert np.isfinite(m.logdensity(x, ignore_prior=True)) or np.isnan(m.logdensity(x, ignore_prior=True))

    bad(lambda x: x.__setitem__(0, m.max_stdev * 1.01))
    bad(lambda x: x.__setitem__(0, -0.1))
    bad(lambda x: x.__setitem__(1, 0.49))
    bad(lambda x: x.__setitem__(1, 2.01))
    # width above max_freq: quad_term2 = 2*2pi*width
    bad(lambda x: x.__setitem__(4, np.log(2 * 2 * np.pi * m.max_freq * 1.01)))
    # width below min_freq on the real root
    bad(lambda x: x.__setitem__(7, np.log(2 * np.pi * m.min_freq * 0.99)))
    # centroids out of order: swap the two quadratic factors
    def swap(x):
        x[3:5], x[5:7] = x[5:7].copy(), x[3:5].copy()
    bad(swap)
    # duplicate roots (fractional difference < 1e-4)
    def dup(x):
        x[5:7] = x[3:5] + 1e-6
    bad(dup)
    # log prior formula (carpack.hpp:118-126)
    assert abs(m.log_prior(th) - (-0.5 * 50 / th[1] - 26.0 * np.log(th[1]))) < 1e-14


def test_chol_update_r1():
    rng = np.random.default_rng(0)
    d = 11
    A = rng.standard_normal((d, d))
    S = A @ A.T + d * np.eye(d)
    R = np.linalg.cholesky(S).T            # upper, S = R^T R (arma::chol convention, steps.cpp:32)
    v = rng.standard_normal(d)
    R2, _ = orc.chol_update_r1(R, v, False)
    np.testing.assert_allclose(R2.T @ R2, S + np.outer(v, v), rtol=1e-12)
    assert np.allclose(R2, np.triu(R2))
    v = 0.1 * v
    R3, _ = orc.chol_update_r1(R, v, True)
    np.testing.assert_allclose(R3.T @ R3, S - np.outer(v, v), rtol=1e-12)


def test_batch_threads_agree(golden_dir):
    g = _load(golden_dir, "carma53_readme.npz")
    m = orc.OracleModel(g["t"], g["y"], g["yerr"], 5, 3)
    a = m.logdensity_batch(g["theta"], nthreads=1)
    b = m.logdensity_batch(g["theta"], nthreads=4)
    np.testing.assert_array_equal(a, b)
    for i in range(4):
        assert a[i] == m.logdensity(g["theta"][i])


def test_predict_matches_reference_python_and_dense_gp(golden_dir):
    """KalmanFilterp::Predict restatement vs KalmanFilterDeprecated.predict (interpolation, at a
    datum, forecast) and vs the dense GP conditional incl. backcasts (carma_unit_tests.cpp:505-649:
    rel 1e-6)."""
    g = _load(golden_dir, "carma53_readme.npz")
    pr = _load(golden_dir, "predict.npz")
    t, y, yerr = g["t"], g["y"], g["yerr"]
    times, back = pr["times"], pr["back"]
    for tag in ("true", "th3", "th17"):
        mu, scale = float(pr[tag + "_mu"]), float(pr[tag + "_scale"])
        args = (t, y - mu, np.sqrt(scale) * yerr, float(pr[tag + "_sigsqr"]), pr[tag + "_omega"], pr[tag + "_ma"])
        m, v = orc.predict_carma(*args, times)
        np.testing.assert_allclose(m, pr[tag + "_pmean"], rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(v, pr[tag + "_pvar"], rtol=1e-9)
        m2, v2 = orc.predict_carma(*args, np.r_[times, back])
        np.testing.assert_allclose(m2, pr[tag + "_dmean"], rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(v2, pr[tag + "_dvar"], rtol=1e-6)
        # forecast variance grows towards the stationary variance
        assert v[-1] > v[-2] > v[-3]


def test_predict_car1_matches_dense_gp(golden_dir):
    """carma_unit_tests.cpp:277-385 (rel 1e-8)."""
    c = _load(golden_dir, "car1_n100.npz")
    pr = _load(golden_dir, "predict.npz")
    th = pr["car1_theta"]
    omega = np.exp(th[3])
    m, v = orc.predict_car1(c["t"], c["y"] - th[2], np.sqrt(th[1]) * c["yerr"], 2 * th[0] ** 2 * omega, omega,
                            pr["car1_times"])
    np.testing.assert_allclose(m, pr["car1_dmean"], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(v, pr["car1_dvar"], rtol=1e-8)


def test_predict_truth_is_tied_to_the_reference_held_vectors(golden_dir):
    """The 50-digit predict reference (mp_truth.predict_truth / predict_truth_car1: the dense Gaussian-process conditional)
    -- the yardstick of tests/test_gpu_model_kernels.py -- against the vectors the REFERENCE's own Python produced
    (tests/golden/make_golden_predict.py): KalmanFilterDeprecated.predict (*_pmean / *_pvar) to 1e-12, its dense solve in
    doubles including the backcasts (*_dmean / *_dvar, car1_*) to 1e-11; means relative to the data's scale.  Then against
    the oracle's Kalman Predict on short series of three orders, all root kinds: 1e-9."""
    from helpers import irregular_series, model_ma, model_roots
    from mp_truth import predict_truth, predict_truth_car1
    g = _load(golden_dir, "carma53_readme.npz")
    pr = _load(golden_dir, "predict.npz")
    t, y, yerr = g["t"], g["y"], g["yerr"]
    times, back = pr["times"], pr["back"]
    nt = times.size
    for tag in ("true", "th3", "th17"):
        mu, scale = float(pr[tag + "_mu"]), float(pr[tag + "_scale"])
        m, v = predict_truth(t, y - mu, np.sqrt(scale) * yerr, float(pr[tag + "_sigsqr"]), pr[tag + "_omega"],
                             pr[tag + "_ma"], np.r_[times, back])
        sc = np.abs(y - mu).max()
        assert np.max(np.abs(m[:nt] - pr[tag + "_pmean"])) <= 1e-12 * sc, tag
        assert np.max(np.abs(v[:nt] - pr[tag + "_pvar"]) / v[:nt]) <= 1e-12, tag
        assert np.max(np.abs(m - pr[tag + "_dmean"])) <= 1e-11 * sc, tag
        assert np.max(np.abs(v - pr[tag + "_dvar"]) / v) <= 1e-11, tag
    c = _load(golden_dir, "car1_n100.npz")
    th = pr["car1_theta"]
    omega = np.exp(th[3])
    m, v = predict_truth_car1(c["t"], c["y"] - th[2], np.sqrt(th[1]) * c["yerr"], 2 * th[0] ** 2 * omega, omega,
                              pr["car1_times"])
    np.testing.assert_allclose(m, pr["car1_dmean"], rtol=1e-11)
    np.testing.assert_allclose(v, pr["car1_dvar"], rtol=1e-11)
    # against the oracle's Kalman Predict (a different algorithm): backcast, datum, midpoint, forecast
    for p, q in ((2, 1), (4, 0), (7, 6)):
        ts, ys, es = irregular_series(40, 10 + p)
        ys = ys - ys.mean()
        tp = np.r_[ts[0] - 30.0, ts[0], ts[5], 0.5 * (ts[9] + ts[10]), ts[-1], ts[-1] + 4.0, ts[-1] + 300.0]
        for kind in ("complex", "real", "mixed"):
            rng = np.random.default_rng(100 * p + q)
            roots, ma = model_roots(rng, p, kind), model_ma(rng, p, q)
            sigsqr = np.var(ys) / orc.variance(roots, ma)
            m, v = predict_truth(ts, ys, es, sigsqr, roots, ma, tp)
            om, ov = orc.predict_carma(ts, ys, es, sigsqr, roots, ma, tp)
            assert np.all(np.abs(om - m) <= 1e-9 * np.maximum(np.abs(m), np.sqrt(v))), (p, q, kind, om, m)
            assert np.all(np.abs(ov - v) <= 1e-9 * v), (p, q, kind, ov, v)
    m, v = predict_truth_car1(ts, ys, es, 0.2, 0.1, tp)
    om, ov = orc.predict_car1(ts, ys, es, 0.2, 0.1, tp)
    assert np.all(np.abs(om - m) <= 1e-9 * np.maximum(np.abs(m), np.sqrt(v))) and np.all(np.abs(ov - v) <= 1e-9 * v)


def test_literal_sampler_restatement_car1(golden_dir):
    """The oracle's restatement of RunCar1Sampler recovers the truth of the CAR(1) fixture
    (carma_unit_tests.cpp:1319-1376 criterion: posterior mean within 3 sigma) and keeps the
    stored-logpost invariant (carma_unit_tests.cpp:783-845)."""
    g = _load(golden_dir, "car1_n100.npz")
    m = orc.OracleModel(g["t"], g["y"], g["yerr"], 1)
    out = m.sampler_run(1, 6000, 6000, 1, 5, g["theta"][0])
    S = out["samples"]
    truth = np.array([2.3, 1.0, 0.0, np.log(0.01)])
    zs = np.abs(S.mean(0) - truth) / S.std(0)
    assert np.all(zs[[0, 2, 3]] < 3.0), zs
    idx = np.arange(0, 6000, 500)
    np.testing.assert_allclose(out["logpost"][idx], m.logdensity_batch(S[idx]), rtol=1e-12)
    assert 0.15 < out["accept_rate"][0] < 0.40


def test_quad_precision_arbiter_is_the_50_digit_value():
    """oracle/carma_truth_q.c (the reference's formulas in __float128: the arbiter of the parity tests) against the
    mpmath restatement at 50 digits (tests/mp_truth.py), on well- and ILL-conditioned models -- including the ones on
    which the double-precision oracle is 1e-5 ... 1e-3 off."""
    from helpers import irregular_series, prior_like_theta
    from mp_truth import loglik_truth as mp_truth
    worst_oracle = 0.0
    for (p, q, picks) in ((2, 1, (0, 1)), (4, 2, (331, 28)), (6, 2, (297, 479)), (6, 1, (849,)), (7, 6, (468, 3)), (5, 3, (767,))):
        t, y, yerr = irregular_series(150, seed=100 * p + q)
        rng = np.random.default_rng(7000 + 10 * p + q)
        th = np.array([prior_like_theta(rng, p, q, t, y) for _ in range(max(picks) + 1)])
        m = orc.OracleModel(t, y, yerr, p, q, max_stdev=10.0 * np.sqrt(np.var(y, ddof=1)))
        for i in picks:
            a, a_ll = orc.truth_logdensity(t, y, yerr, th[i], p, q)
            b, b_ll = mp_truth(t, y, yerr, th[i], p, q)
            assert abs(a - b) <= 4e-16 * abs(b) and abs(a_ll - b_ll) <= 4e-16 * abs(b_ll), (p, q, i, a, b)
            o = m.logdensity(th[i], ignore_prior=True)
            if np.isfinite(o):
                worst_oracle = max(worst_oracle, abs(o - b) / abs(b))
    assert worst_oracle > 1e-6          # these cases ARE the ones the double-precision restatement cannot resolve


def test_ogle_grid_car1_member(golden_dir):
    """(p, q) = (1, 0) on OGLE-LMC-LPV-00007 (the 28th order of BASELINE configs[4]): the oracle's CAR(1) filter and
    log-density against the closed-form dense Gaussian process (make_golden_ogle_car1.py)."""
    og = np.loadtxt(os.path.join(golden_dir, "ogle_lmc_lpv_00007.dat"))
    t, y, e = og[:, 0], og[:, 1], og[:, 2]
    g = _load(golden_dir, "ogle_car1.npz")
    m = orc.OracleModel(t, y, e, 1)
    for i, th in enumerate(g["theta"]):
        mean, var = orc.kfilter_car1(t, y - th[2], np.sqrt(th[1]) * e, 2.0 * th[0] ** 2 * np.exp(th[3]), np.exp(th[3]))
        np.testing.assert_allclose(var, g["var"][i], rtol=1e-9)
        np.testing.assert_allclose(mean, g["mean"][i], rtol=0, atol=1e-9 * np.abs(y - th[2]).max())
        ll = m.logdensity(th) - m.log_prior(th)
        assert np.isfinite(ll) and abs(ll - g["loglik"][i]) <= 1e-10 * abs(ll)
        assert abs(ll - g["dense_loglik"][i]) <= 1e-9 * abs(ll)


def test_arbiter_is_tied_to_the_reference_held_vectors(golden_dir):
    """The quad-precision arbiter (oracle/carma_truth_q.c) -- which the parity tests consult wherever the GPU and the
    oracle disagree -- against the log-likelihoods the REFERENCE's own Python produced (KalmanFilterDeprecated,
    tests/golden/make_golden.py): every README CARMA(5,3) vector and every OGLE (p, q) vector.  The reference computes in
    double precision through an LU solve, so its distance from the exact value grows with cond(EigenMat): 1e-13 on
    everything below cond 1e5, 2e-12 at worst (measured 1.2e-12 at cond 3.8e5)."""
    g = _load(golden_dir, "carma53_readme.npz")
    t, y, e = g["t"], g["y"], g["yerr"]
    worst = 0.0
    for i, th in enumerate(g["theta"]):
        ll = orc.truth_logdensity(t, y, e, th, 5, 3)[1]
        r = abs(ll - g["loglik"][i]) / abs(ll)
        assert r <= 1e-13, (i, r, g["cond"][i])
        worst = max(worst, r)
    og = _load(golden_dir, "ogle_grid.npz")
    t, y, e = og["t"], og["y"], og["yerr"]
    for p in range(2, 8):
        for q in range(p):
            k = "p%dq%d_" % (p, q)
            for i, th in enumerate(og[k + "theta"]):
                ll = orc.truth_logdensity(t, y, e, th, p, q)[1]
                r = abs(ll - og[k + "loglik"][i]) / abs(ll)
                assert r <= (1e-13 if og[k + "cond"][i] < 1e5 else 2e-12), (p, q, i, r, og[k + "cond"][i])
                worst = max(worst, r)
    print("arbiter vs reference-held log-likelihoods: worst %.2e over 113 vectors" % worst)


def test_oracle_on_the_config3_series(golden_dir):
    """BASELINE configs[3] at its full size -- CARMA(7,6), n = 10 000, time steps 0.1 + |Cauchy| -- against
    KalmanFilterDeprecated (tests/golden/make_golden_hard.py): log-likelihood and the strided Kalman mean / variance
    for the generating parameters, two posterior-like neighbours and two prior-like draws (one with cond 6e11)."""
    g = _load(golden_dir, "config3_carma76_n10000.npz")
    t, y, e = g["t"], g["y"], g["yerr"]
    p, q, stride = int(g["p"]), int(g["q"]), int(g["stride"])
    m = orc.OracleModel(t, y, e, p, q)
    for i, th in enumerate(g["theta"]):
        ll = m.logdensity(th, ignore_prior=True) - m.log_prior(th)
        assert abs(ll - g["loglik"][i]) <= 1e-12 * abs(ll), (i, ll, g["loglik"][i])
        om, ma = orc.ar_roots(th, p), orc.ma_coefs(th, p, q)
        mean, var = orc.kfilter_carma(t, y - th[2], np.sqrt(th[1]) * e, th[0] ** 2 / orc.variance(om, ma), om, ma)
        np.testing.assert_allclose(var[::stride], g["var"][i], rtol=1e-9)
        np.testing.assert_allclose(mean[::stride], g["mean"][i], rtol=0, atol=1e-9 * np.abs(y - th[2]).max())
        truth = orc.truth_logdensity(t, y, e, th, p, q)[1]
        assert abs(truth - g["loglik"][i]) <= 1e-13 * abs(truth)


def test_distance_of_the_oracle_from_the_reference_on_ill_conditioned_models(golden_dir):
    """36 parameter vectors with cond(EigenMat) from 2e3 to 3e12 (25 of them above 1e6; make_golden_hard.py): the oracle
    restates the reference's LU solve operation by operation, but LAPACK's pivoting and blocking are its own, so on
    these inputs the two double-precision computations part ways -- by as much as each of them differs from the exact
    value of the formulas.  What is asserted: (1) below cond 1e5 the oracle matches the reference to 1e-11; (2)
    everywhere the oracle is no more than 30x further from the exact (quad-precision) value than the reference is, or
    within 1e-12 of it; (3) the disagreement itself stays below 1e-4 (worst on record: 6.6e-6 at cond 1.2e8).  The
    table is printed so that the distance is on record."""
    g = _load(golden_dir, "illcond_readme.npz")
    t, y, e = g["t"], g["y"], g["yerr"]
    n_above = 0
    worst = (0.0, 0.0)
    for i in range(len(g["p"])):
        p, q = int(g["p"][i]), int(g["q"][i])
        th = g["theta"][i][: 3 + p + q]
        m = orc.OracleModel(t, y, e, p, q)
        o = m.logdensity(th, ignore_prior=True) - m.log_prior(th)
        ref = float(g["loglik"][i])
        truth = orc.truth_logdensity(t, y, e, th, p, q)[1]
        d_or, d_ot, d_rt = abs(o - ref) / abs(ref), abs(o - truth) / abs(truth), abs(ref - truth) / abs(truth)
        print("p=%d q=%d cond %.1e: oracle-reference %.1e | oracle-exact %.1e  reference-exact %.1e" % (
            p, q, g["cond"][i], d_or, d_ot, d_rt))
        if g["cond"][i] < 1e5:
            assert d_or <= 1e-11, (i, d_or)
        assert d_ot <= max(30.0 * d_rt, 1e-12), (i, d_ot, d_rt)
        assert d_or <= 1e-4, (i, d_or)
        n_above += g["cond"][i] >= 1e6
        if d_or > worst[0]:
            worst = (d_or, float(g["cond"][i]))
    assert n_above >= 20
    print("worst oracle-reference distance %.1e at cond %.1e" % worst)


def test_zero_root_band_states(golden_dir):
    """Two states the GPU sampler stored in the configs[2] run (round 3) on which the REFERENCE's arithmetic gives NaN by a
    rounding accident: an MA quadratic factor with two real roots and 4 q1 / q2^2 = 2^-52.25 / 2^-52.07, where the
    reference's smaller root -(q2 - sqrt(q2^2 - 4 q1)) / 2 comes out as exactly zero and its MA polynomial divides by it
    (carpack.cpp:522-580).  The exact value of the formulas is finite (quad precision), the device reproduced it to 1e-15
    -- with the last bit of exp() the coin can land either way, which is what helpers.in_zero_root_band excuses."""
    from helpers import in_zero_root_band
    g = _load(golden_dir, "carma53_readme.npz")
    t, y, e = g["t"], g["y"], g["yerr"]
    ms = 10.0 * np.sqrt(np.mean(y * y) - np.mean(y) ** 2)
    m = orc.OracleModel(t, y, e, 5, 3, max_stdev=ms)
    states = [
        ([2.3521415749979684, 1.1353751202125038, 16.346713997289932, -2.6070758477523803, -3.4086607253064884, -3.7678557418618164,
          1.01437543843715, -3.4723410470074025, 23.141959232799465, 30.37101444163148, 108.3259598958267], -117.74892595616718),
        ([1.729609217076725, 1.548875058116524, 16.159812169772717, -2.6234816883436123, -2.798166309693116, -7.57636705521334,
          -2.833068476446049, 0.6623614004138593, -3.4957159671186826, 16.992497163911835, 231.87726605878635], -122.07286251511061),
    ]
    for th, device_value in states:
        th = np.array(th)
        assert in_zero_root_band(th, 5, 3) and m.check_prior_bounds(th)
        assert np.isnan(m.logdensity(th))                                  # the reference's own NaN
        truth = orc.truth_logdensity(t, y, e, th, 5, 3)[0]
        assert np.isfinite(truth) and abs(device_value - truth) <= 1e-13 * abs(truth)
    assert not in_zero_root_band(g["theta"][0], 5, 3)


def test_overflow_region_states():
    """Two states the row sampler's hottest chains reached after 1e5 iterations (tools/soak_pt_row.py, round 3): MA roots of
    1e-80, i.e. MA coefficients of 1e232 / 1e212.  The reference's variance sum overflows (carpack.cpp:377-409: inf - inf),
    its log-density is NaN; the exact value of the formulas is finite; the device, whose products overflow to a signed
    infinity instead, returned the finite artefacts below.  helpers.in_overflow_region marks such states; a state with MA
    coefficients of 1e140 is not one of them and the oracle is still accurate there."""
    from helpers import in_overflow_region, irregular_series
    cases = [
        (5, 3, 150, [17.22824544342013, 1.2745485191040822, 30.631556629773975, 3.3215189525138253, 0.04152298407997157, -2.1710738002768433,
                     -3.0652113134025343, -3.1860764607521013, -431.8271481828337, -227.4478231315038, -102.69653144548043], -500.49841724813194),
        (6, 5, 180, [9.287673296489519, 0.9496851981974919, 14.052320089691424, 2.836598980825528, -0.9118708180562727, -2.173393918906031,
                     -0.39659888619471284, -2.5189781815345054, 0.4605053478983999, -388.83945708097895, -451.6081396505746, -99.91149364880701,
                     -221.60789424027953, 48.86365195573411], -438.4889889274666),
    ]
    for p, q, n, th, device_value in cases:
        t, y, e = irregular_series(n, seed=11 * p + q)
        th = np.array(th)
        m = orc.OracleModel(t, y, e, p, q, max_stdev=10.0 * np.sqrt(np.mean(y * y) - np.mean(y) ** 2))
        assert in_overflow_region(th, p, q)
        assert np.max(np.abs(orc.ma_coefs(th, p, q))) > 1e200
        assert np.isnan(m.logdensity(th, ignore_prior=True))
        truth = orc.truth_logdensity(t, y, e, th, p, q)[0]
        assert np.isfinite(truth) and abs(device_value - truth) > 1e-4 * abs(truth)
    # 1e140: large, yet the arithmetic holds
    t, y, e = irregular_series(150, seed=58)
    th = np.array([17.2, 1.27, 30.6, 3.32, 0.0415, -2.17, -3.07, -3.19, -322.0, -150.0, -1.0])
    assert 1e135 < np.max(np.abs(orc.ma_coefs(th, 5, 3))) < 1e150 and not in_overflow_region(th, 5, 3)
    m = orc.OracleModel(t, y, e, 5, 3, max_stdev=1e3)
    got, truth = m.logdensity(th, ignore_prior=True), orc.truth_logdensity(t, y, e, th, 5, 3)[0]
    assert np.isfinite(got) and abs(got - truth) <= 1e-6 * abs(truth), (got, truth)


def test_filter_arbiter_is_tied_to_the_reference_held_vectors(golden_dir):
    """oracle.truth_filter (quad-precision mean[n] / var[n], the arbiter of the mean / variance comparisons) against the
    reference Python's own vectors: README CARMA(5,3), every stored parameter vector, <= 1e-12; and on the ill-conditioned
    set its distance from the reference's LAPACK LU grows with cond(EigenMat) as the log-likelihood's does."""
    g = _load(golden_dir, "carma53_readme.npz")
    t, y, e = g["t"], g["y"], g["yerr"]
    worst = 0.0
    for i in range(g["theta"].shape[0]):
        if not np.all(np.isfinite(g["var"][i])):
            continue
        m, v = orc.truth_filter(t, y, e, g["theta"][i], 5, 3)
        worst = max(worst, np.max(np.abs(v - g["var"][i]) / g["var"][i]), np.max(np.abs(m - g["mean"][i])) / np.abs(y).max())
    assert worst <= 1e-12, worst
    h = _load(golden_dir, "illcond_readme.npz")
    low = [i for i in range(len(h["p"])) if h["cond"][i] < 1e5]
    for i in low:
        p, q = int(h["p"][i]), int(h["q"][i])
        m, v = orc.truth_filter(h["t"], h["y"], h["yerr"], h["theta"][i][: 3 + p + q], p, q)
        assert np.max(np.abs(v - h["var"][i]) / h["var"][i]) <= 1e-9, (i, h["cond"][i])
