"""GPU tests of the multi-band log-density (k_logdens_carma_mband behind carma_bands_*) and of the fits built on it
(CarmaBandsModel.get_mle / lag_profile).  The references and the case table are tests/mband_ref.py's; tests/test_mband_cpu.py holds
kalman_ref to the exact value on every input first, so the bound below -- the project's 1e-10 -- needs no arbitration."""
import os

import numpy as np
import pytest

import mband_ref as R
from helpers import prior_like_theta, theta_batch

pytestmark = pytest.mark.gpu
RTOL = 1e-10


@pytest.fixture(scope="module")
def cpa():
    import carma_pack_amd
    assert carma_pack_amd._lib.lib.carma_device_count() >= 1
    return carma_pack_amd


def _rel(got, want):
    return np.max(np.abs(np.asarray(got) - np.asarray(want)) / np.abs(want))


def _boxes(thx, d, K, pad=1.0):
    """A lag box around the lags the rows of thx hold."""
    lags = np.atleast_2d(thx)[:, d + 3 * np.arange(K - 1)]
    return np.c_[lags.min(axis=0) - pad, lags.max(axis=0) + pad]


# ---- the kernel against the exact value -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q,name", R.CASES)
def test_kernel_vs_dense_truth(cpa, p, q, name):
    bands, thx, truth = R.case(p, q, name)
    K = len(bands)
    assert sum(len(b[0]) for b in bands) <= 40 and thx.shape[0] <= 24
    ctx = cpa.BandsContext(bands, p, q, lag_bounds=_boxes(thx, 3 + p + q, K))
    assert ctx.nbands == K and ctx.dx == thx.shape[1] and list(ctx.n) == [len(b[0]) for b in bands]
    got = ctx.logdensity(thx, ignore_prior=True) - R.log_prior(thx[:, 1])
    print("%s (%d,%d): device %r exact %r rel %.2e" % (name, p, q, got, truth, _rel(got, truth)))
    assert np.all(np.isfinite(got))
    assert _rel(got, truth) <= RTOL
    one = ctx.logdensity(thx[1], ignore_prior=True)          # a single vector: a float, the same bits
    assert isinstance(one, float) and one == ctx.logdensity(thx, ignore_prior=True)[1]
    ctx.close()


# ---- lanes of one wave on different merge orders ----------------------------------------------------------------------------------
LANE_P, LANE_Q = 5, 3


def _lane_problem():
    rng = np.random.default_rng(77)
    bands = []
    for b in range(3):
        t = np.cumsum(rng.uniform(0.5, 2.5, 200)) + 3.0 * b
        bands.append((t, 1.0 * b + (1.0 + 0.5 * b) * np.sin(t / 9.0 + b) + 0.3 * rng.standard_normal(200), rng.uniform(0.1, 0.3, 200)))
    th = R.order_thetas(LANE_P, LANE_Q)
    thx = np.empty((130, 3 + LANE_P + LANE_Q + 6))
    for i in range(130):
        base = th[i % 2].copy()
        base[:3] += [0.1 * rng.uniform(), 0.05 * rng.uniform(), 0.2 * rng.standard_normal()]
        thx[i] = R.extend(base, [(rng.uniform(-40.0, 40.0), 1.0 + rng.uniform(), 1.0 + 0.3 * rng.standard_normal()),
                                 (rng.uniform(-40.0, 40.0), 1.5 + rng.uniform(), 2.0 + 0.3 * rng.standard_normal())])
    return bands, thx


@pytest.fixture(scope="module")
def lane_problem():
    bands, thx = _lane_problem()
    return bands, thx, R.kalman_ref(bands, thx, LANE_P, LANE_Q) + R.log_prior(thx[:, 1])     # once, for every B


@pytest.mark.parametrize("B", [1, 63, 65, 130])
def test_lanes_are_independent(cpa, lane_problem, B):
    """A different random lag per lane (+-40 on bands that span ~300: the merge orders differ all along the walk), B on both sides
    of a wave: every lane gets the value of ITS vector, whatever its neighbours do."""
    bands, thx, want = lane_problem
    assert [len(b[0]) for b in bands] == [200, 200, 200]
    ctx = cpa.BandsContext(bands, LANE_P, LANE_Q, lag_bounds=[(-50.0, 50.0)] * 2)
    got = ctx.logdensity(thx[:B], ignore_prior=True)
    print("B = %d: max rel difference from kalman_ref %.2e" % (B, _rel(got, want[:B])))
    assert _rel(got, want[:B]) <= RTOL
    # the same vectors in another place of the batch: the same bits
    if B > 1:
        perm = np.random.default_rng(B).permutation(B)
        assert np.array_equal(ctx.logdensity(thx[:B][perm], ignore_prior=True), got[perm])
    ctx.close()


# ---- one band: the single-series entry point ------------------------------------------------------------------------------------
def test_one_band_vs_single_series_call(cpa, golden_dir):
    g = np.load(os.path.join(golden_dir, "carma53_readme.npz"))
    t, y, yerr = g["t"], g["y"], g["yerr"]
    th = theta_batch(np.random.default_rng(0), 64, 5, 3, t, y, theta_center=g["theta"][0])
    ms = 10.0 * np.sqrt(np.mean(y * y) - np.mean(y) ** 2)
    one = cpa.Context(t, y, yerr, 5, 3, max_stdev=ms)
    ctx = cpa.BandsContext([(t, y, yerr)], 5, 3, max_stdev=ms)
    assert ctx.dx == one.d and ctx.prior() == one.prior()
    for ignore in (False, True):
        want, got = one.logdensity(th, ignore_prior=ignore), ctx.logdensity(th, ignore_prior=ignore)
        fin = np.isfinite(want)
        assert fin.sum() >= 32
        assert np.array_equal(np.isfinite(got), fin) and np.array_equal(np.isneginf(got), np.isneginf(want))
        print("ignore_prior=%d: %d finite, max rel difference %.2e" % (ignore, fin.sum(), _rel(got[fin], want[fin])))
        assert _rel(got[fin], want[fin]) <= RTOL
    ctx.close()
    one.close()


# ---- the prior ---------------------------------------------------------------------------------------------------------------------
def test_prior_pattern(cpa):
    p, q = 3, 1
    d = 3 + p + q
    bands, extras = R.scenario("three_bands_7_1_12", seed=3)
    t0, y0, e0 = bands[0]
    rng = np.random.default_rng(5)
    th = np.array([prior_like_theta(rng, p, q, t0, y0) for _ in range(96)])
    th[::7, 0] = 1e3                                         # ysigma above max_stdev
    th[3::11, 1] = 2.5                                       # measerr_scale above 2
    th[5::13, 3] = 9.0                                       # a frequency above max_freq
    ms = 10.0 * y0.std()
    one = cpa.Context(t0, y0, e0, p, q, max_stdev=ms)
    ctx = cpa.BandsContext(bands, p, q, lag_bounds=[(0.0, 2.0), (-1.0, 1.0)], max_stdev=ms)
    assert ctx.prior() == one.prior()
    thx = np.array([R.extend(x, extras) for x in th])
    want = one.logdensity(th)
    got = ctx.logdensity(thx)
    assert 8 <= np.isneginf(want).sum() <= 88                # both kinds are present
    assert np.array_equal(np.isneginf(got), np.isneginf(want))         # the CARMA part: band 0's own pattern
    ok = np.flatnonzero(np.isfinite(got))
    x = thx[ok[0]]
    rows = np.tile(x, (7, 1))
    rows[1, d] = 2.5                                         # lag 1 above its box
    rows[2, d + 3] = -1.0000001                              # lag 2 below its box
    rows[3, d + 3] = np.nan
    rows[4, d + 1] = np.nan                                  # log a
    rows[5, d + 5] = np.inf                                  # mu of band 2
    rows[6, d] = 0.0                                         # on the edge: inside
    got = ctx.logdensity(rows)
    assert np.array_equal(np.isneginf(got), [False, True, True, True, True, True, False]) and np.isfinite(got[[0, 6]]).all()
    got = ctx.logdensity(rows, ignore_prior=True)            # the boxes are part of the prior; a non-finite entry is -inf regardless
    assert np.array_equal(np.isneginf(got), [False, False, False, True, True, True, False])
    ctx.close()
    one.close()


# ---- the caller's order, and nothing beyond it ------------------------------------------------------------------------------------
def test_pad_lanes_write_nothing(cpa):
    import torch
    p, q = 2, 1
    bands, thx, _ = R.case(p, q, "eight_bands")
    ctx = cpa.BandsContext(bands, p, q, lag_bounds=_boxes(thx, 3 + p + q, 8))
    rng = np.random.default_rng(1)
    B = 65                                                   # the second wave holds one live lane and 63 pad lanes
    rows = np.tile(thx[0], (B, 1))
    rows[:, 2] += rng.standard_normal(B)                     # every row its own value
    want = ctx.logdensity(rows, ignore_prior=True)
    assert np.unique(want).size == B
    dev = torch.device("cuda")
    d_th = torch.from_numpy(rows).to(dev)
    out = torch.full((192,), -12345.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.logdensity_dev(d_th.data_ptr(), B, out.data_ptr(), ignore_prior=True, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:B], want)
    assert np.all(got[B:] == -12345.0)
    ctx.close()


def test_mle_argument_errors_on_a_live_handle(cpa):
    bands, thx, _ = R.case(2, 1, "lag_equals_offset")
    ctx = cpa.BandsContext(bands, 2, 1, lag_bounds=[(0.0, 5.0)])
    with pytest.raises(ValueError):
        ctx.mle_batched(thx, mem=0)
    with pytest.raises(ValueError):
        ctx.mle_batched(thx, maxiter=-1)
    with pytest.raises(ValueError):
        ctx.mle_batched(thx, fixed_lag=np.array([[1.0], [np.nan]]))
    lo = np.full(ctx.dx, -np.inf)
    lo[6] = 6.0                                              # above the lag box
    with pytest.raises(ValueError):
        ctx.mle_batched(thx, lo=lo)
    ctx.close()


# ---- fits ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recovery(cpa):
    bands, x_true = R.recovery_problem()
    model = cpa.CarmaBandsModel(bands, p=2, q=1, lag_bounds=[(-1.0, 9.0)])
    return bands, x_true, model


def test_lag_profile_recovers_the_lag(cpa, recovery):
    bands, x_true, model = recovery
    lags = R.RECOVERY_LAGS.copy()
    prof, xs = model.lag_profile(lags, ntrials=8, seed=11)
    print("profile log-likelihood over the lags %s: %s" % (lags, np.round(prof, 2)))
    assert prof.shape == (9,) and xs.shape == (9, model.dx) and np.all(np.isfinite(prof))
    assert lags[int(np.argmax(prof))] == R.RECOVERY_TRUE_LAG
    assert xs[:, model.d].tobytes() == lags.tobytes()        # the lags come back bit-identical
    # every profile value is the likelihood AT the optimum it comes with ...
    assert np.allclose(model.loglik(xs), prof, rtol=1e-12, atol=0)
    # ... and at least the likelihood of every start it was reached from (the starts of lag_profile, that row's lag put in)
    x0, _, _ = model._starts(8, 11)
    for k, lag in enumerate(lags):
        st = x0.copy()
        st[:, model.d] = lag
        f0 = model.loglik(st)
        f0 = f0[np.isfinite(f0)]
        assert f0.size and prof[k] >= f0.max()
    # at the true lag the fit is at least as good as the parameters the data were drawn from, and the scale is recovered
    assert prof[4] >= model.loglik(x_true)
    assert abs(np.exp(xs[4, model.d + 1]) - 2.0) < 0.1


def test_get_mle_vs_scipy_on_kalman_ref(cpa, recovery):
    """The criterion of test_config4_choose_order_vs_scipy for a smooth low order: the lock-step optimum is no worse than what
    scipy's L-BFGS-B reaches on the float64 reference objective from the SAME (best) start, to 0.05 in -log L."""
    from scipy.optimize import minimize
    bands, x_true, model = recovery
    res = model.get_mle(ntrials=16, seed=11, return_all=True)
    funs = np.array([r.fun if np.isfinite(r.fun) else 1e300 for r in res])
    best = int(np.argmin(funs))
    assert funs[best] < 1e299
    one = model.get_mle(ntrials=16, seed=11)
    assert one.fun == funs[best] and np.array_equal(one.x, res[best].x)
    lag = one.x[model.d]
    assert -1.0 <= lag <= 9.0
    # the objective is the reference's: -(kalman_ref + log prior of the error scale) at the optimum
    fg = R.neg_logpost_and_grad(bands, 2, 1)
    assert abs(fg(one.x)[0] - one.fun) <= 1e-9 * abs(one.fun)
    x0, lo, hi = model._starts(16, 11)
    lo[model.d], hi[model.d] = -1.0, 9.0
    ref = minimize(fg, np.clip(x0[best], lo, hi), jac=True, method="L-BFGS-B", bounds=list(zip(lo, hi)))
    print("get_mle: -log L %.4f at lag %.4f (start %d of 16) | scipy on kalman_ref from the same start: %.4f at lag %.4f" % (
        one.fun, lag, best, ref.fun, ref.x[model.d]))
    assert one.fun <= ref.fun + 0.05
