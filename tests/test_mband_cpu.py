"""CPU-only tests of the multi-band code: the two references against each other, the lane filter that merges the bands
(carma_mband.h, built for the host: tests/emu/emu_mband.cpp) against the exact value, the argument checks of the C ABI, and the
evaluator that puts fixed lags into the optimiser's points (carma_mband_plan.h) on an objective with a known answer."""
import ctypes as C
import os

import numpy as np
import pytest

import carma_pack_amd as cpa
import emu_build
import helpers
import mband_build as mb
import mband_ref as R

L = cpa._lib.lib
EINVAL = -22
RTOL = 1e-10        # the project's parity bound; every input here is well conditioned (cond(EigenMat) < 1e5)
_dp = C.POINTER(C.c_double)


def _rel(got, want):
    return np.max(np.abs(np.asarray(got) - np.asarray(want)) / np.abs(want))


# ---- the inputs, before anything else ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q", R.ORDERS)
def test_root_sets_are_well_conditioned(p, q):
    for th in R.order_thetas(p, q):
        assert th.size == 3 + p + q
        if p > 1:
            assert helpers.cond_eigenmat(th, p) < 1e5
    if p >= 2:   # the second root set holds a quadratic factor with two real roots
        lq = R.order_thetas(p, q)[1][3:3 + p]
        assert any(np.exp(2 * lq[2 * i + 1]) > 4 * np.exp(lq[2 * i]) for i in range(p // 2))


def test_scenarios_are_what_they_claim():
    ties = lambda tau: int(np.sum(np.diff(tau) == 0))                            # noqa: E731
    for p, _ in R.ORDERS:
        for name in R.SCENARIOS:
            bands, extras = R.scenario(name, seed=p)
            assert 2 <= sum(len(b[0]) for b in bands) <= 40
            for t, _, _ in bands:
                assert np.all(np.diff(t) > 0)
            tau, band, _ = R.merge_order(bands, [0.0] + [e[0] for e in extras])
            if name == "lag0_shared_stamps":
                assert extras[0][0] == 0.0 and ties(tau) == 8
            if name == "lag_equals_offset":
                assert extras[0][0] != 0.0 and ties(tau) == 9
            if name == "band1_first":
                assert band[0] == 1 and np.all(band[:9] == 1) and np.all(band[9:] == 0)
            if name == "disjoint_after":
                assert np.all(band[:12] == 0) and np.all(band[12:] == 1)
            if name == "three_bands_7_1_12":
                assert [len(b[0]) for b in bands] == [7, 1, 12] and np.any(np.diff(band) != 0)
            if name == "eight_bands":
                assert len(bands) == 8 and all(2 <= len(b[0]) <= 5 for b in bands) and ties(tau) >= 1
            # on a tie the lower band goes first
            eq = np.flatnonzero(np.diff(tau) == 0)
            assert np.all(band[eq] < band[eq + 1])


@pytest.mark.parametrize("p,q,name", R.CASES)
def test_kalman_ref_agrees_with_dense_truth(p, q, name):
    """The condition the GPU tests' use of kalman_ref rests on: within 1e-10 relative of the exact value on EVERY input."""
    bands, thx, truth = R.case(p, q, name)
    got = [R.kalman_ref(bands, x, p, q) for x in thx]
    assert _rel(got, truth) <= RTOL


# ---- the lane filter -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q,name", R.CASES)
def test_lane_filter_vs_dense_truth(p, q, name):
    bands, thx, truth = R.case(p, q, name)
    got = mb.logdensity(bands, p, q, thx, ignore_prior=True) - R.log_prior(thx[:, 1])
    assert np.all(np.isfinite(got))
    assert _rel(got, truth) <= RTOL, (got, truth)


def test_result_does_not_depend_on_the_order_of_equal_bands_parameters():
    """Two bands that swap places (with the parameters that go with them) give the same likelihood when nothing ties."""
    bands, extras = R.scenario("three_bands_7_1_12", seed=3)
    th = R.order_thetas(3, 0)[0]
    a = mb.logdensity(bands, 3, 0, R.extend(th, extras))
    b = mb.logdensity([bands[0], bands[2], bands[1]], 3, 0, R.extend(th, [extras[1], extras[0]]))
    assert _rel(a, b) <= 1e-12


@pytest.mark.parametrize("p,q", [(2, 1), (3, 0), (4, 2), (5, 3), (6, 0), (7, 6)])
def test_one_band_equals_single_series_lane_filter(p, q):
    t, y, yerr = helpers.irregular_series(60, 5)
    rng = np.random.default_rng(p)
    th = helpers.theta_batch(rng, 12, p, q, t, y, theta_center=helpers.prior_like_theta(np.random.default_rng(1), p, q, t, y))
    prior = (10.0 * y.std(), 1.0 / np.diff(t).min(), 1.0 / (t[-1] - t[0]))
    for ignore in (True, False):
        want = emu_build.logdensity_carma_lane(t, y, yerr, p, q, th, prior, ignore_prior=ignore)
        got = mb.logdensity([(t, y, yerr)], p, q, th, prior=prior, ignore_prior=ignore)
        assert np.array_equal(np.isneginf(got), np.isneginf(want))
        fin = np.isfinite(want)
        assert fin.sum() >= (12 if ignore else 1)
        assert np.array_equal(np.isfinite(got), fin)
        assert _rel(got[fin], want[fin]) <= 1e-12


def test_one_band_car1_equals_single_series_car1():
    t, y, yerr = helpers.irregular_series(60, 6)
    rng = np.random.default_rng(2)
    th = np.array([helpers.prior_like_theta(rng, 1, 0, t, y) for _ in range(12)])
    th[0, 3] = 5.0                                           # omega above max_freq: -inf on both sides
    prior = (10.0 * y.std(), 1.0 / np.diff(t).min(), 1.0 / (t[-1] - t[0]))
    want = emu_build.logdensity_car1(t, y, yerr, th, prior)
    got = mb.logdensity([(t, y, yerr)], 1, 0, th, prior=prior, ignore_prior=False)
    assert np.isneginf(want[0]) and np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert fin.sum() >= 8 and _rel(got[fin], want[fin]) <= 1e-12


def test_prior_of_the_band_parameters():
    bands, extras = R.scenario("three_bands_7_1_12", seed=2)
    th = R.order_thetas(2, 1)[0]
    prior = (1e3, 1e3, 1e-6)
    box = [(0.0, 2.0), (-1.0, 1.0)]
    x = R.extend(th, extras)
    rows = np.tile(x, (8, 1))
    d = 3 + 2 + 1
    rows[1, d] = 2.5                                         # lag 1 above its box
    rows[2, d + 3] = -1.5                                    # lag 2 below its box
    rows[3, d] = np.nan
    rows[4, d + 1] = np.inf                                  # log a
    rows[5, d + 5] = -np.inf                                 # mu of band 2
    rows[6, d + 4] = np.nan                                  # log a of band 2
    rows[7, d] = 2.0                                         # on the edge of the box: inside
    got = mb.logdensity(bands, 2, 1, rows, lag_bounds=box, prior=prior, ignore_prior=False)
    assert np.array_equal(np.isneginf(got), [False, True, True, True, True, True, True, False])
    assert np.isfinite(got[0]) and np.isfinite(got[7])
    # without the prior the boxes are not tested; a non-finite entry is still -inf
    got = mb.logdensity(bands, 2, 1, rows, lag_bounds=box, prior=prior, ignore_prior=True)
    assert np.array_equal(np.isneginf(got), [False, False, False, True, True, True, True, False])
    want = R.dense_truth(bands, rows[1], 2, 1) + R.log_prior(rows[1, 1])
    assert abs(got[1] - want) <= RTOL * abs(want)


# ---- C ABI: argument errors without a GPU ----------------------------------------------------------------------------------------
def _create(bands, p, q, lo, hi, K=None):
    t, y, e, off = R.flat(bands)
    lo = None if lo is None else np.ascontiguousarray(lo, dtype=float)
    hi = None if hi is None else np.ascontiguousarray(hi, dtype=float)
    h = L.carma_bands_create(t.ctypes.data_as(_dp), y.ctypes.data_as(_dp), e.ctypes.data_as(_dp), off.ctypes.data_as(C.POINTER(C.c_long)),
                             len(bands) if K is None else K, p, q, None if lo is None else lo.ctypes.data_as(_dp),
                             None if hi is None else hi.ctypes.data_as(_dp), 10.0, 0)
    msg = cpa._lib.last_error()
    if h:
        L.carma_bands_destroy(h)
    return h, msg


def test_bands_create_argument_errors_before_device_work():
    t = np.arange(6.0)
    b = (t, np.sin(t), np.full(6, 0.1))
    one = (t[:1], t[:1], t[:1] + 1)
    empty = (t[:0], t[:0], t[:0])
    bad = [
        (([b, b], 2, 0, None, None), "lag_lo"),                          # boxes missing
        (([b, b], 2, 0, [1.0], [0.0]), "lag box"),                       # lo > hi
        (([b, b], 2, 0, [np.nan], [1.0]), "lag box"),
        (([b, b], 2, 2, [0.0], [1.0]), "q < p"),
        (([b, b], 0, 0, [0.0], [1.0]), "q < p"),
        (([b, b], 8, 0, [0.0], [1.0]), "q < p"),
        (([b, empty], 2, 0, [0.0], [1.0]), "band 1 is empty"),
        (([one], 1, 0, None, None), "at least 2"),
        (([b] * 9, 2, 0, [0.0] * 8, [1.0] * 8), "nbands"),
        (([b], 2, 0, None, None, 0), "nbands"),
        (([(t, np.where(t == 3, np.inf, t), t + 1), b], 2, 0, [0.0], [1.0]), "not finite"),
    ]
    for args, word in bad:
        h, msg = _create(*args)
        assert not h and word in msg and "no HIP device" not in msg, (word, msg)
    # the same checks as a return code (carma_mband_plan.h): CARMA_EINVAL
    H = mb.mle_host()
    buf = C.create_string_buffer(256)
    tt, yy, ee, off = R.flat([b, empty])
    lo, hi = np.zeros(1), np.ones(1)
    assert H.mband_check_create_host(tt.ctypes.data_as(_dp), yy.ctypes.data_as(_dp), ee.ctypes.data_as(_dp),
                                     off.ctypes.data_as(C.POINTER(C.c_long)), 2, 2, 0, lo.ctypes.data_as(_dp), hi.ctypes.data_as(_dp),
                                     buf, 256) == EINVAL
    tt, yy, ee, off = R.flat([b, one])
    assert H.mband_check_create_host(tt.ctypes.data_as(_dp), yy.ctypes.data_as(_dp), ee.ctypes.data_as(_dp),
                                     off.ctypes.data_as(C.POINTER(C.c_long)), 2, 2, 0, lo.ctypes.data_as(_dp), hi.ctypes.data_as(_dp),
                                     buf, 256) == 0 and buf.value == b""
    if L.carma_device_count() == 0:                          # a valid call gets as far as the device
        h, msg = _create([b, one], 2, 0, [0.0], [1.0])
        assert not h and "no HIP device" in msg
        with pytest.raises(cpa.CarmaDeviceError):
            cpa.BandsContext([b, one], 2, 0, lag_bounds=[(0.0, 1.0)])
    with pytest.raises(ValueError):
        cpa.BandsContext([b, b], 2, 0)                       # no lag box for the second band
    with pytest.raises(ValueError):
        cpa.BandsContext([b, empty], 2, 0, lag_bounds=[(0.0, 1.0)])


def test_null_handles_and_mle_arguments_are_einval():
    x = np.zeros(16)
    vp = x.ctypes.data_as(C.c_void_p)
    assert L.carma_bands_dim(None) == EINVAL
    assert L.carma_bands_nbands(None) == EINVAL
    assert L.carma_bands_n(None, 0) == EINVAL
    assert L.carma_bands_get_prior(None, x.ctypes.data_as(_dp)) == EINVAL
    assert L.carma_bands_logdensity_batch(None, x.ctypes.data_as(_dp), 1, 0, x.ctypes.data_as(_dp)) == EINVAL
    assert L.carma_bands_logdensity_batch_dev(None, vp, 1, 0, vp, None) == EINVAL
    assert L.carma_bands_mle_batched(None, vp, 1, None, None, None, 10, 8, 1e-9, 1e-5, 1e-6, 1, vp, vp, None, None, None) == EINVAL
    L.carma_bands_destroy(None)


def test_python_model_input_checks_and_merged():
    t = np.array([3.0, 1.0, 2.0, 2.0])
    b0 = (t, np.array([30.0, 10.0, 20.0, 21.0]), np.full(4, 0.5))
    b1 = (np.array([1.5, 4.0]), np.array([7.0, 9.0]), np.array([0.2, 0.4]))
    with pytest.raises(ValueError):
        cpa.CarmaBandsModel([b0, b1], p=1, q=1)
    with pytest.raises(ValueError):
        cpa.CarmaBandsModel([b0, b1], p=2, q=0, lag_bounds=[(0, 1), (0, 1)])
    m = cpa.CarmaBandsModel([b0, b1], p=2, q=1, lag_bounds=[(-3.0, 3.0)])
    assert m.K == 2 and m.dx == 3 + 2 + 1 + 3
    assert np.array_equal(m.bands[0][0], [1.0, 2.0, 3.0]) and np.array_equal(m.bands[0][1], [10.0, 20.0, 30.0])
    theta = np.array([1.0, 1.0, 5.0, 0.1, 0.2, 0.3, -0.5, np.log(2.0), 1.0])
    tm, ym, em, band = m.merged(theta)
    assert np.array_equal(tm, [1.0, 2.0, 2.0, 3.0, 4.5])     # 1.5 + 0.5 ties with band 0's 2.0 and goes after it
    assert np.array_equal(band, [0, 0, 1, 0, 1])
    assert np.allclose(ym, [10.0, 20.0, (7.0 - 1.0) / 2.0 + 5.0, 30.0, (9.0 - 1.0) / 2.0 + 5.0], rtol=1e-15)
    assert np.allclose(em, [0.5, 0.5, 0.1, 0.5, 0.2], rtol=1e-15)
    assert "equal times" in cpa.CarmaBandsModel.merged.__doc__
    with pytest.raises(ValueError):
        m.lag_profile([5.0])                                 # outside the box: refused before any device work


def test_built_harness_libraries_are_git_ignored():
    pats = [ln.strip() for ln in open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), ".gitignore"))]
    assert "*.so" in pats                                    # tests/emu/libcarma_emu_mband.so, tests/mband/libmband_mle_host.so
    assert mb.EMU_SO.endswith(".so") and mb.MLE_SO.endswith(".so")


# ---- the evaluator's fixed-lag insertion, through mle_loop -------------------------------------------------------------------
def test_fixed_lags_are_inserted_per_start_and_never_optimised():
    """log-density -sum_j w_j (x_j - c_j - s)^2 over the variables that are not lags, s = the sum of the point's lags: the optimum
    of a start is c + (the sum of ITS fixed lags), so a lag of another start -- or the lag entry of x0 -- in any point shows."""
    d, K = 4, 3
    dx = d + 3 * (K - 1)
    lagc = [d, d + 3]
    free = [j for j in range(dx) if j not in lagc]
    c = np.linspace(-1.0, 1.0, dx)
    w = np.linspace(1.0, 3.0, dx)

    def dens(thx):
        s = thx[:, lagc].sum(axis=1)
        return -np.sum(w[free] * (thx[:, free] - c[free] - s[:, None]) ** 2, axis=1)

    B = 5
    rng = np.random.default_rng(0)
    fixed = np.array([[0.0, 0.0], [1.0, -0.25], [0.1, 0.2], [-2.0, 0.5], [0.3, 0.3]])
    x0 = rng.normal(size=(B, dx))
    x0[:, lagc] = 99.0                                       # must never be read
    lo, hi = np.full(dx, -np.inf), np.full(dx, np.inf)
    lo[lagc], hi[lagc] = 7.0, 7.0                            # ... nor these: an empty box would give the stencil no width
    x, f, status, calls = mb.mle(dens, d, K, x0, lo, hi, fixed_lag=fixed)
    assert np.all(status < 2)
    assert np.array_equal(x[:, lagc], fixed)                 # bit-identical
    want = c[free][None, :] + fixed.sum(axis=1)[:, None]
    assert np.max(np.abs(x[:, free] - want)) < 1e-5
    assert np.max(np.abs(f)) < 1e-9
    rows = {tuple(r) for r in fixed}
    assert calls and all(tuple(r) in rows for pts in calls for r in pts[:, lagc])
    # every stencil moves one FREE variable: no point differs from its centre in a lag
    first = calls[0].reshape(B, 2 * (dx - 2) + 1, dx)
    assert np.all(first[:, :, lagc] == fixed[:, None, :])
    assert np.all(np.sum(first[:, 1:, :] != first[:, :1, :], axis=2) == 1)


def test_free_lags_are_optimised_inside_their_box():
    d, K = 4, 2
    dx = d + 3
    c = np.array([0.5, -0.5, 1.0, 2.0, 3.0, 0.25, -1.0])     # the lag's optimum 3.0 lies above its box

    def dens(thx):
        return -np.sum((thx - c) ** 2, axis=1)

    lo, hi = np.full(dx, -np.inf), np.full(dx, np.inf)
    lo[d], hi[d] = -1.0, 2.0
    x, f, status, calls = mb.mle(dens, d, K, np.zeros((3, dx)) + np.array([[0.0], [0.5], [-0.5]]), lo, hi)
    assert np.all(status < 2)
    want = c.copy()
    want[d] = 2.0
    assert np.max(np.abs(x - want)) < 1e-5
    assert np.allclose(f, 1.0, atol=1e-8)
    assert all(pts.shape[1] == dx and np.all((pts[:, d] >= -1.0) & (pts[:, d] <= 2.0)) for pts in calls)


# ---- the lag-recovery problem of the GPU tests: its own reference must recover the lag ----------------------------------------
def test_kalman_ref_profile_peaks_at_the_true_lag():
    bands, x_true = R.recovery_problem()
    assert [len(b[0]) for b in bands] == [60, 60] and x_true[3 + 2 + 1] == R.RECOVERY_TRUE_LAG
    prof = R.kalman_profile(bands, x_true, R.RECOVERY_LAGS)
    k = int(np.argmax(prof))
    assert R.RECOVERY_LAGS[k] == R.RECOVERY_TRUE_LAG
    assert prof[k] - np.delete(prof, k).max() > 10.0         # by a wide margin in log-likelihood, not by luck
