"""GPU tests of the multi-band smoother (k_smooth_mband_fwd / _bwd behind carma_bands_smooth, BandsContext.smooth,
CarmaBandsModel.smooth / smooth_band).  The references, the case table and the bound are tests/mband_smooth_ref.py's;
tests/test_mband_smooth_cpu.py holds the header's host build and kalman_smooth_ref to the exact value on every input first.
The bound is the project's smoother rule: 1e-9 for every entry, means relative to max(|mean|, sd), variances relative to the exact
variance."""
import ctypes as C

import numpy as np
import pytest

import mband_ref as R
import mband_smooth_ref as S
import smooth_ref as sr
from test_gpu_mband import LANE_P, LANE_Q, _lane_problem

pytestmark = pytest.mark.gpu
CARMA_EINVAL = -22


@pytest.fixture(scope="module")
def cpa():
    import carma_pack_amd
    assert carma_pack_amd._lib.lib.carma_device_count() >= 1
    return carma_pack_amd


def _boxes(thx, d, K, pad=1.0):
    lags = np.atleast_2d(thx)[:, d + 3 * np.arange(K - 1)]
    return np.c_[lags.min(axis=0) - pad, lags.max(axis=0) + pad]


def _bits(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ---- the kernels against the exact value --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q,name", R.CASES)
def test_kernels_vs_dense_truth(cpa, p, q, name):
    bands, thx, table = S.smooth_case(p, q, name)
    K = len(bands)
    ctx = cpa.BandsContext(bands, p, q, lag_bounds=_boxes(thx, 3 + p + q, K))
    for bo, (tout, tm, tv) in table.items():
        mean, var, inv = ctx.smooth(thx, bo, tout)
        em, ev = S.errors(mean, var, tm, tv)
        print("%s (%d,%d) band %d: device from the exact value: mean %.2e var %.2e" % (name, p, q, bo, em, ev))
        assert mean.shape == var.shape == (2, 12) and inv.shape == (2,) and not inv.any()
        assert np.all(np.isfinite(mean)) and np.all(np.isfinite(var))
        assert em <= S.RTOL and ev <= S.RTOL
        i, j = np.flatnonzero(tout == tout[np.argmax([np.sum(tout == v) for v in tout])])
        assert np.array_equal(mean[:, i], mean[:, j]) and np.array_equal(var[:, i], var[:, j])   # the repeated time: equal bits
        m1, v1, i1 = ctx.smooth(thx[1], bo, tout)            # a single vector: the bits of its row in the batch
        assert m1.shape == v1.shape == (12,) and i1 is False
        assert np.array_equal(m1, mean[1]) and np.array_equal(v1, var[1])
    ctx.close()


# ---- lanes of one wave on different merge orders, launch edges --------------------------------------------------------------------------
LANE_BAND, LANE_M = 1, 40


@pytest.fixture(scope="module")
def lane_problem():
    bands, thx = _lane_problem()
    rng = np.random.default_rng(40)
    lo, hi = min(t[0] for t, _, _ in bands), max(t[-1] for t, _, _ in bands)
    tout = rng.uniform(lo - 30.0, hi + 30.0, LANE_M)         # (inside and beyond the data of every lane's merge)
    tout[7] = tout[3]
    return bands, thx, tout, S.kalman_smooth_ref(bands, thx, LANE_P, LANE_Q, LANE_BAND, tout)   # once, for every B


@pytest.mark.parametrize("B", [1, 63, 65, 130])
def test_lanes_and_launch_edges(cpa, lane_problem, B):
    """The problem of test_lanes_are_independent (a random lag per lane, +-40 on bands that span ~300), B on both sides of a wave:
    every lane gets the curve of ITS vector, wherever it sits in the batch and however the call is cut into chunks."""
    bands, thx, tout, (wm, wv) = lane_problem
    assert [len(b[0]) for b in bands] == [200, 200, 200] and tout.size == 40
    lib = cpa._lib
    ctx = cpa.BandsContext(bands, LANE_P, LANE_Q, lag_bounds=[(-50.0, 50.0)] * 2)
    got = ctx.smooth(thx[:B], LANE_BAND, tout)
    assert not got[2].any()
    em, ev = S.errors(got[0], got[1], wm[:B], wv[:B])
    print("B = %d: from kalman_smooth_ref: mean %.2e var %.2e" % (B, em, ev))
    assert em <= S.RTOL and ev <= S.RTOL
    if B > 1:
        perm = np.random.default_rng(B).permutation(B)
        again = ctx.smooth(thx[:B][perm], LANE_BAND, tout)
        assert _bits(again, [g[perm] for g in got])
    try:
        for rows in (64, 1):
            lib.tune_set("MBAND_SMOOTH_CHUNK_ROWS", rows)
            assert _bits(ctx.smooth(thx[:B], LANE_BAND, tout), got), rows
    finally:
        lib.tune_set("MBAND_SMOOTH_CHUNK_ROWS", None)
    ctx.close()


# ---- one band: the single-series smoother -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q", [(2, 1), (5, 3), (7, 6)])
def test_one_band_vs_smooth_carma(cpa, p, q):
    """A BandsContext of one band against smooth_carma of the same models on the same series (another arithmetic: agreement within
    the bound, not bits).  smooth_carma takes yerr as given, so it gets yerr sqrt(measerr_scale)."""
    from carma_pack_amd.carma_pack import mle_to_model
    rng = np.random.default_rng(48 + p)
    t = np.cumsum(rng.uniform(0.3, 2.0, 48))
    y = 0.4 + np.sin(t / 5.0) + 0.2 * rng.standard_normal(48)
    yerr = rng.uniform(0.1, 0.3, 48)
    tout = np.concatenate([rng.uniform(t[0] - 5.0, t[-1] + 5.0, 30), t[[3, 20]]])
    thx = np.array(R.order_thetas(p, q))
    ctx = cpa.BandsContext([(t, y, yerr)], p, q)
    mean, var, inv = ctx.smooth(thx, 0, tout)
    assert not inv.any()
    for k in range(2):
        sig, roots, ma, mu = mle_to_model(thx[k], p, q)
        wm, wv = cpa._lib.smooth_carma(t, y, yerr * np.sqrt(thx[k, 1]), [sig], [roots], [ma], [mu], tout)
        em, ev = S.errors(mean[k], var[k], wm[0], wv[0])
        print("p = %d row %d: from smooth_carma: mean %.2e var %.2e" % (p, k, em, ev))
        assert em <= S.RTOL and ev <= S.RTOL
    ctx.close()


# ---- the relation between the bands' curves ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lag_equals_offset", "three_bands_7_1_12"])
@pytest.mark.parametrize("p,q", R.ORDERS)
def test_band_relation(cpa, p, q, name):
    """Times and lags on the grid of 1/4 (1/16): t + lag_b is exact, so band b at t + lag_b and band 0 at t are the same point of
    the same walk, and mean_b = a_b (mean_0 - mu_0) + mu_b, var_b = a_b^2 var_0 up to the rounding of those few operations:
    1e-12, the mean in units of max(|mean_b|, sd_b) (a mean may cancel to 0), the variance relative."""
    bands, thx, _ = R.case(p, q, name)
    K, d = len(bands), 3 + p + q
    lo, hi = min(t[0] for t, _, _ in bands), max(t[-1] for t, _, _ in bands)
    t = np.arange(lo - 2.0, hi + 2.0, 0.75)
    ctx = cpa.BandsContext(bands, p, q, lag_bounds=_boxes(thx, d, K))
    m0, v0, _ = ctx.smooth(thx, 0, t)
    for b in range(1, K):
        lag = thx[0, d + 3 * (b - 1)]
        assert np.all(thx[:, d + 3 * (b - 1)] == lag) and np.all((t + lag) - lag == t)
        a, mub = np.exp(thx[:, d + 3 * (b - 1) + 1])[:, None], thx[:, d + 3 * (b - 1) + 2][:, None]
        mb, vb, inv = ctx.smooth(thx, b, t + lag)
        assert not inv.any()
        wm, wv = a * (m0 - thx[:, 2][:, None]) + mub, a * a * v0
        em = np.max(np.abs(mb - wm) / np.maximum(np.abs(wm), np.sqrt(wv)))
        ev = np.max(np.abs(vb - wv) / wv)
        print("%s (%d,%d) band %d: relation holds to mean %.2e var %.2e" % (name, p, q, b, em, ev))
        assert em <= 1e-12 and ev <= 1e-12
    ctx.close()


# ---- the mixture ---------------------------------------------------------------------------------------------------------------------------------
def _assert_band(bm, bv, m, v, keep=None):
    """4 K 2^-53 of the sum of |terms| per entry: the bound of a K-term ordered sum (tests/test_gpu_smooth.py)."""
    rm, rvv, am, av = sr.band_moments(m, v, keep)
    K = m.shape[0] if keep is None else int(np.sum(keep))
    eps = 4.0 * K * 2.0 ** -53
    assert np.all(np.abs(bm - rm) <= eps * am), np.max(np.abs(bm - rm) / am)
    assert np.all(np.abs(bv - rvv) <= eps * av), np.max(np.abs(bv - rvv) / av)


def _mixture_rows(B, seed):
    bands, thx, _ = R.case(3, 0, "three_bands_7_1_12")
    rng = np.random.default_rng(seed)
    rows = np.tile(thx[0], (B, 1))
    rows[:, 2] += 0.1 * rng.standard_normal(B)
    rows[:, 6] += rng.uniform(-0.5, 0.5, B)                   # the lag of band 1
    return bands, rows


@pytest.mark.parametrize("B", (1, 5, 67))
def test_mixture_of_the_calls_own_rows(cpa, B):
    bands, rows = _mixture_rows(B, B)
    tout = np.linspace(-3.0, 30.0, 25)
    ctx = cpa.BandsContext(bands, 3, 0, lag_bounds=[(-5.0, 5.0)] * 2)
    m, v, bm, bv, inv = ctx.smooth(rows, 2, tout, moments=True)
    assert m.shape == (B, 25) and bm.shape == bv.shape == (25,) and not inv.any()
    _assert_band(bm, bv, m, v)
    assert _bits(ctx.smooth(rows, 2, tout), (m, v, inv))      # with or without the mixture: the same rows
    ctx.close()


def test_invalid_row_is_flagged_and_left_out(cpa):
    bands, rows = _mixture_rows(6, 9)
    rows[4, 6] = np.nan                                       # the lag of band 1
    tout = np.linspace(-3.0, 30.0, 25)
    ctx = cpa.BandsContext(bands, 3, 0, lag_bounds=[(-5.0, 5.0)] * 2)
    m, v, bm, bv, inv = ctx.smooth(rows, 0, tout, moments=True)
    assert list(inv) == [False] * 4 + [True, False]
    assert np.all(np.isnan(m[4])) and np.all(np.isnan(v[4])) and np.all(np.isfinite(np.delete(m, 4, axis=0)))
    _assert_band(bm, bv, m, v, keep=~inv)
    good = np.delete(rows, 4, axis=0)
    assert _bits(ctx.smooth(good, 0, tout), (np.delete(m, 4, axis=0), np.delete(v, 4, axis=0), np.delete(inv, 4)))
    # at the C level without the flag array: the call returns 1
    lib = cpa._lib
    mm, vv = np.empty((6, 25)), np.empty((6, 25))
    rc = lib.lib.carma_bands_smooth(ctx._h, lib.ptr(rows), 6, 0, lib.ptr(tout), 25, lib.ptr(mm), lib.ptr(vv), None, None, None)
    assert rc == 1 and _bits((mm, vv), (m, v))
    assert lib.lib.carma_bands_smooth(ctx._h, lib.ptr(good), 5, 0, lib.ptr(tout), 25, lib.ptr(mm), lib.ptr(vv), None, None, None) == 0
    ctx.close()


# ---- argument errors ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(cpa):
    lib = cpa._lib
    bands, rows = _mixture_rows(3, 1)
    tout = np.array([4.0, -1.0, 11.5, 4.0])
    ctx = cpa.BandsContext(bands, 3, 0, lag_bounds=[(-5.0, 5.0)] * 2)
    before = ctx.smooth(rows, 1, tout, moments=True)
    m, v, bm, bv = np.empty((3, 4)), np.empty((3, 4)), np.empty(4), np.empty(4)
    inv = np.zeros(3, dtype=np.int32)
    P = lib.ptr
    bad_t = tout.copy()
    bad_t[2] = np.inf
    nan_t = tout.copy()
    nan_t[0] = np.nan

    def call(h=ctx._h, th=P(rows), B=3, band=1, t=P(tout), M=4, mean=P(m), var=P(v), bmean=None, bvar=None):
        return lib.lib.carma_bands_smooth(h, th, B, band, t, M, mean, var, bmean, bvar, inv.ctypes.data_as(C.POINTER(C.c_int)))

    cases = [(dict(h=None), "null handle"), (dict(B=0), "need B >= 1"), (dict(M=0), "M >= 1"), (dict(band=-1), "band -1"),
             (dict(band=3), "band 3 is outside [0, 3)"), (dict(t=P(bad_t)), "tout[2] is not finite"),
             (dict(t=P(nan_t)), "tout[0] is not finite"), (dict(var=None), "pairs"), (dict(bmean=P(bm)), "pairs"),
             (dict(mean=None, var=None), "one pair at least"), (dict(th=None), "non-null"), (dict(t=None), "non-null")]
    for kw, text in cases:
        assert call(**kw) == CARMA_EINVAL, kw
        msg = lib.last_error()
        assert msg.startswith("carma_bands_smooth: ") and text in msg, (kw, msg)
    with pytest.raises(ValueError, match="band 7"):
        ctx.smooth(rows, 7, tout)
    assert call(mean=None, var=None, bmean=P(bm), bvar=P(bv)) == 0                      # the mixture alone is a legal call
    assert _bits(ctx.smooth(rows, 1, tout, moments=True), before)                       # ... and the handle is as it was
    assert _bits((bm, bv), before[2:4])
    ctx.close()


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------------------
def test_python_layer(cpa):
    from carma_pack_amd.carma_pack import CarmaBandsModel
    bands, x = R.recovery_problem()
    model = CarmaBandsModel(bands, p=2, q=1, lag_bounds=[(0.0, 8.0)])
    d = 6
    xs = np.tile(x, (3, 1))
    xs[1, d] -= 1.0
    xs[2, d] += 1.0
    time = np.linspace(bands[1][0][0] - 5.0, bands[1][0][-1] + 5.0, 50)
    for band in (0, 1):
        m1, v1 = model.smooth(x, time, band=band)
        m3, v3 = model.smooth(xs, time, band=band)
        assert m1.shape == v1.shape == (50,) and m3.shape == v3.shape == (3, 50)
        assert np.array_equal(m1, m3[0]) and np.array_equal(v1, v3[0])
        assert np.all(v3 > 0) and not np.array_equal(m3[0], m3[1]) and not np.array_equal(m3[0], m3[2])
        wm, wv = S.kalman_smooth_ref(bands, xs, 2, 1, band, time)
        em, ev = S.errors(m3, v3, wm, wv)
        print("recovery problem band %d: from kalman_smooth_ref: mean %.2e var %.2e" % (band, em, ev))
        assert em <= S.RTOL and ev <= S.RTOL
        bm, bv = model.smooth_band(xs, time, band=band)
        assert bm.shape == bv.shape == (50,)
        _assert_band(bm, bv, m3, v3)
    # at the vector the data were drawn from, band 1's curve passes its own data within the errors: 1 % noise
    t1, y1, e1 = bands[1]
    mfit, vfit = model.smooth(x, t1, band=1)
    assert np.max(np.abs(mfit - y1) / e1) < 6.0
    assert "smooth" in CarmaBandsModel.merged.__doc__
    bad = xs.copy()
    bad[1, d + 1] = np.nan
    with pytest.raises(ValueError, match="row 1"):
        model.smooth(bad, time)
    with pytest.raises(ValueError, match="row 1"):
        model.smooth_band(bad, time, band=1)
