"""GPU tests of the sampler of a multi-band fit (carma_bands_pt_*, BandsContext.pt_*, CarmaBandsModel.run_mcmc) and of the wide RAM
bookkeeping kernels (k_ram_propose_wide / k_ram_finish_wide).

The yardstick of a trajectory is the REFERENCE LADDER (tests/mband_pt_build.py: ram_propose / ram_finish / exchange_sweep of
carma_pt_core.h on the host, at any dimension) fed with the context's own pt_logdensity: both sides then see the same log-density
bits and only the bookkeeping is under test.

Starting values.  The rows of mband_ref.case() lie OUTSIDE the prior of band 0 of their scenarios (their AR widths are below
min_freq = 1 / span of a band of 5 ... 12 data): their log-posterior is -inf, and a chain that starts at -inf never accepts
(steps.cpp:41-46).  The trajectory tests therefore take the CARMA part from the reference's starting-value distribution on band 0
(a seeded numpy generator: nothing depends on the library's drawn starts) and the band terms from the scenario, with small jitter.

Largest deviations observed against the reference ladder are printed by the tests and recorded in NOTEBOOK.md."""
import ctypes as C
import os

import numpy as np
import pytest

import mband_pt_build as pb
import mband_pt_ref as ptref
import mband_ref as R
from helpers import irregular_series, prior_like_theta

pytestmark = pytest.mark.gpu

SEED = 20240923
RTOL, ATOL = 1e-6, 1e-9          # test_lane_kernel_walks_the_ladder_kernels_trajectory's bound


@pytest.fixture(scope="module")
def cpa():
    import carma_pack_amd
    assert carma_pack_amd._lib.lib.carma_device_count() >= 1, "no MI355X visible"
    return carma_pack_amd


_CTX = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    """The module's contexts (and their sampler buffers) go when its last test is done."""
    yield
    for item in _CTX.values():
        item[0].close()
    _CTX.clear()


def _problem(cpa, p, q, name):
    """(ctx, bands, extras, lag_bounds, box) of a scenario at an order, one context per module."""
    key = (p, q, name)
    if key not in _CTX:
        bands, extras = R.scenario(name, seed=p)
        bands = pb.prepared(bands)
        lb = np.array([(e[0] - 1.0, e[0] + 1.0) for e in extras])
        ctx = cpa.BandsContext(bands, p, q, lag_bounds=lb, max_stdev=ptref.prior3(bands)[0])
        # the default box, widened to hold the scenario's own band terms (a band of one or two data need not contain its level)
        lo, hi = ctx.pt_default_box()
        np.testing.assert_allclose(np.array([lo, hi]), np.array(pb.default_box(bands)), rtol=1e-13, atol=0)
        val = np.array([(np.log(e[1]), e[2]) for e in extras])
        _CTX[key] = (ctx, bands, extras, lb, (np.minimum(lo, val - 1.0), np.maximum(hi, val + 1.0)))
    return _CTX[key]


def _points(rng, n, p, q, bands, extras, jitter=1e-3):
    """n extended vectors inside the prior of band 0 (mostly): prior-like CARMA parts, the scenario's band terms, jittered."""
    t0, y0, _ = bands[0]
    x = np.array([R.extend(prior_like_theta(rng, p, q, t0, y0), extras) for _ in range(n)])
    return x + jitter * rng.standard_normal(x.shape)


def _temps(T):
    return np.exp(np.log(100.0) * np.arange(T) / max(T - 1, 1))


ORDERS = [(1, 0), (2, 1), (5, 3), (7, 6)]
SCENARIOS = ["lag0_shared_stamps", "three_bands_7_1_12", "eight_bands"]


# ---- 1. K1 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENARIOS)
@pytest.mark.parametrize("p,q", ORDERS)
def test_k1_has_the_bits_of_the_batch_kernel_and_the_box(cpa, p, q, name):
    ctx, bands, extras, lb, box = _problem(cpa, p, q, name)
    K, d, dx = len(bands), ctx.d, ctx.dx
    assert dx == 3 + p + q + 3 * (K - 1) <= 37
    rng = np.random.default_rng(100 * p + q + K)
    case_rows = np.array([R.extend(th, extras) for th in R.order_thetas(p, q)])
    for T, Rr in ((10, 2), (3, 5), (64, 1)):
        ctx.pt_create(T, Rr, 5, seed=1, band_box=box)
        assert ctx.pt_kernel_name() == "k_logdens_carma_mband_chains<%d>" % p
        nc = T * Rr
        assert T == 64 or nc % 64 != 0                       # a partly filled wave
        th = _points(rng, nc, p, q, bands, extras)
        half = len(th[::2])
        th[::2] = case_rows[np.arange(half) % 2] + 1e-3 * rng.standard_normal((half, dx))   # (the finite ones at p = 1)
        inside = th.copy()
        # outside: a lag past its box (the library's own prior), log a and mu past the band box, one NaN
        th[1, d] = lb[0, 1] + 0.5
        th[3, d + 1] = box[1][0, 0] + 1e-6
        th[5, d + 3 * (K - 2) + 2] = box[0][K - 2, 1] - 1e-6
        th[7, d + 1] = np.nan
        got = ctx.pt_logdensity(th.reshape(Rr, T, dx)).ravel()
        want = ctx.logdensity(inside, ignore_prior=False)
        touched = np.array([1, 3, 5, 7])
        rest = np.setdiff1d(np.arange(nc), touched)
        assert np.array_equal(got[rest], want[rest]), (T, Rr, np.flatnonzero(got[rest] != want[rest])[:4])
        assert np.all(np.isneginf(got[touched]))
        assert np.isfinite(got).any() and np.isneginf(got).any()
        # on the edge of the band box: inside
        edge = inside[rest[np.isfinite(want[rest])][:1]].repeat(nc, axis=0)
        edge[0, d + 1], edge[1, d + 2] = box[0][0, 0], box[1][0, 1]
        ge = ctx.pt_logdensity(edge.reshape(Rr, T, dx)).ravel()
        assert np.array_equal(ge, ctx.logdensity(edge, ignore_prior=False)) and np.isfinite(ge[:2]).all()
        # no box: nothing but the library's log-density (the guard words behind the results are checked by the entry point)
        ctx.pt_create(T, Rr, 5, seed=1)
        th[7, d + 1] = inside[7, d + 1]
        assert np.array_equal(ctx.pt_logdensity(th.reshape(Rr, T, dx)).ravel(), ctx.logdensity(th, ignore_prior=False))


# ---- 2. the trajectory against the reference ladder -----------------------------------------------------------------------------
TRAJ = [(2, 1, "lag0_shared_stamps", pb.RAM_FUSED), (5, 2, "lag0_shared_stamps", pb.RAM_SPLIT),
        (5, 3, "three_bands_7_1_12", pb.RAM_WIDE), (7, 6, "eight_bands", pb.RAM_WIDE)]


def _counts(ctx):
    a, w = ctx.pt_stats()
    n = ctx.pt_iterations_done()
    return np.rint(a * n).astype(np.int64), np.rint(w * n).astype(np.int64)


def _walk(ctx, adapt, frozen, ns, thin):
    ctx.pt_iterate(adapt + frozen, True)
    th1, lp1 = ctx.pt_get_chains()
    f1 = ctx.pt_get_factor()
    sm, sl = ctx.pt_sample(ns, thin)
    th2, lp2 = ctx.pt_get_chains()
    return dict(th1=th1, lp1=lp1, f1=f1, sm=sm, sl=sl, th2=th2, lp2=lp2, f2=ctx.pt_get_factor(), counts=_counts(ctx))


@pytest.mark.parametrize("T,Rr", [(3, 3), (10, 3), (64, 1)])
@pytest.mark.parametrize("p,q,name,kind", TRAJ)
def test_sampler_walks_the_reference_ladders_trajectory(cpa, p, q, name, kind, T, Rr):
    ctx, bands, extras, lb, box = _problem(cpa, p, q, name)
    dx = ctx.dx
    assert dx == {pb.RAM_FUSED: 9, pb.RAM_SPLIT: 13}.get(kind, dx) and pb.ram_kernels_plan(dx) == kind
    adapt, frozen = 25, 40
    rng = np.random.default_rng(7 * dx + T)
    ctx.pt_create(T, Rr, adapt, seed=SEED, temperatures=_temps(T), band_box=box)
    # every chain starts at a finite log-posterior (a chain at -inf never moves, and the two sweeps treat inf - inf differently:
    # exchange_sweep's fmin(exp(NaN), 1) accepts, exchange_decide's comparison with a NaN rejects)
    start = _points(rng, Rr * T, p, q, bands, extras)
    for _ in range(20):
        bad = ~(np.isfinite(ctx.logdensity(start, ignore_prior=False)) & pb.in_box(start, ctx.d, len(bands), box))
        if not bad.any():
            break
        start[bad] = _points(rng, int(bad.sum()), p, q, bands, extras)
    ctx.pt_set_chains(start.reshape(Rr, T, dx))
    th0, lp0 = ctx.pt_get_chains()
    assert np.all(np.isfinite(lp0))
    f0 = ctx.pt_get_factor()
    np.testing.assert_allclose(f0, np.broadcast_to(pb.initial_factor(bands, ctx.d), f0.shape), rtol=1e-13, atol=0)
    lad = pb.Ladder(lambda x: ctx.pt_logdensity(x.reshape(Rr, T, dx)).ravel(), dx, T, Rr, adapt, SEED, th0, lp0, f0, temps=_temps(T))
    g = _walk(ctx, adapt, frozen, 5, 3)
    lad.iterate(adapt + frozen)
    th1, lp1, f1 = lad.theta.copy(), lad.lp.copy(), lad.chol.copy()
    sm, sl = lad.sample(5, 3)
    assert ctx.pt_iterations_done() == lad.iter == adapt + frozen + 15
    assert np.array_equal(g["counts"][0], lad.nacc) and np.array_equal(g["counts"][1], lad.nswap)
    assert lad.nacc.sum() > 0 and (T == 1 or lad.nswap.sum() > 0)
    pairs = [(g["th1"], th1), (g["lp1"], lp1), (g["f1"], f1), (g["sm"], sm), (g["sl"], sl), (g["th2"], lad.theta), (g["lp2"], lad.lp),
             (g["f2"], lad.chol)]
    dev = max(float(np.max(np.abs(a - b) / (ATOL / RTOL + np.abs(b)))) for a, b in pairs)
    print("dx=%d T=%d R=%d: largest deviation from the reference ladder %.3e (relative, floor %.0e)" % (dx, T, Rr, dev, ATOL / RTOL))
    for a, b in pairs:
        np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL)
    assert not np.array_equal(g["th1"], th0) and not np.array_equal(g["f1"], f0)


# ---- 3. the wide kernels against the templated ones, on the existing samplers --------------------------------------------------------
def _with_wide(cpa, run):
    """run() with the tune entry at its default and at 4 (every d through the wide kernels) -> both results."""
    a = run()
    try:
        cpa._lib.tune_set("PT_RAM_WIDE_MIN", 4)
        b = run()
    finally:
        cpa._lib.tune_set("PT_RAM_WIDE_MIN", None)
    return a, b


def _compare_wide(tag, a, b):
    assert np.array_equal(a["counts"][0], b["counts"][0]) and np.array_equal(a["counts"][1], b["counts"][1]), tag
    keys = ("th1", "lp1", "f1", "sm", "sl", "th2", "lp2", "f2")
    exact = all(np.array_equal(a[k], b[k]) for k in keys)
    dev = max(float(np.max(np.abs(a[k] - b[k]) / (ATOL / RTOL + np.abs(a[k])))) for k in keys)
    print("%s: wide against templated: %s (largest deviation %.3e)" % (tag, "bit-identical" if exact else "NOT bit-identical", dev))
    for k in keys:
        np.testing.assert_allclose(b[k], a[k], rtol=RTOL, atol=ATOL, err_msg="%s %s" % (tag, k))
    assert a["counts"][0].sum() > 0


@pytest.mark.parametrize("p,q", [(1, 0), (2, 1), (5, 3), (7, 6)])
def test_wide_kernels_walk_the_templated_kernels_trajectory(cpa, p, q):
    t, y, e = irregular_series(100, seed=40 + p)
    ctx = cpa.Context(t, y, e, p, q)
    assert ctx.d == {1: 4, 2: 6, 5: 11, 7: 16}[p]
    old = os.environ.get("CARMA_PT_KERNEL")
    os.environ["CARMA_PT_KERNEL"] = "lane"
    try:
        def run():
            ctx.pt_create(10, 7, 25, seed=SEED)
            assert ctx.pt_kernel() == "lane"
            ctx.pt_start()
            return _walk(ctx, 25, 40, 5, 3)
        a, b = _with_wide(cpa, run)
    finally:
        if old is None:
            del os.environ["CARMA_PT_KERNEL"]
        else:
            os.environ["CARMA_PT_KERNEL"] = old
    _compare_wide("Context d=%d" % ctx.d, a, b)
    ctx.close()


def test_wide_kernels_walk_the_multi_series_samplers_trajectory(cpa):
    sset = [irregular_series(n, seed=70 + i) for i, n in enumerate([40, 90, 64])]
    mc = cpa.MultiContext(sset, 3, 1)

    def run():
        mc.pt_create([2, 0, 1, 0], 10, 2, 25, seed=SEED)
        mc.pt_start()
        return _walk(mc, 25, 40, 5, 3)
    a, b = _with_wide(cpa, run)
    _compare_wide("MultiContext d=%d" % mc.d, a, b)
    mc.close()


# ---- 4. self-consistency, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q,name", [(2, 1, "lag0_shared_stamps"), (5, 3, "three_bands_7_1_12")])
def test_chunks_seeds_and_replicas(cpa, p, q, name):
    ctx, bands, extras, lb, box = _problem(cpa, p, q, name)
    T, Rr = 10, 3

    def run(seed, parts, samples):
        ctx.pt_create(T, Rr, 30, seed=seed, band_box=box)
        ctx.pt_start()
        for n in parts:
            ctx.pt_iterate(n, True)
        out = [ctx.pt_sample(n, 2) for n in samples]
        th, lp = ctx.pt_get_chains()
        return th, lp, ctx.pt_get_factor(), np.concatenate([o[0] for o in out], axis=1), np.concatenate([o[1] for o in out], axis=1)

    a = run(SEED, [40], [11])
    for other in (run(SEED, [13, 27], [8, 3]), run(SEED, [40], [11])):
        for x, y in zip(a, other):
            assert np.array_equal(x, y)
    c = run(SEED + 1, [40], [11])
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[3], c[3])
    assert a[3].shape == (Rr, 11, ctx.dx)
    for i in range(Rr):
        for j in range(i):
            assert not np.array_equal(a[3][i], a[3][j])      # replicas differ from each other


# ---- 5. starts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q,name", [(2, 1, "lag0_shared_stamps"), (5, 3, "three_bands_7_1_12"), (7, 6, "eight_bands")])
def test_starting_values(cpa, p, q, name):
    ctx, bands, extras, lb, box = _problem(cpa, p, q, name)
    K, d, dx = len(bands), ctx.d, ctx.dx
    T, Rr = 10, 2
    ctx.pt_create(T, Rr, 5, seed=SEED, band_box=box)
    ctx.pt_start()
    th, lp = ctx.pt_get_chains()
    flat = th.reshape(-1, dx)
    assert np.all(np.isfinite(flat)) and np.all(np.isfinite(lp))
    cols = d + 3 * np.arange(K - 1)
    assert np.all((flat[:, cols] >= lb[:, 0]) & (flat[:, cols] <= lb[:, 1])) and pb.in_box(flat, d, K, box).all()
    assert np.array_equal(lp.ravel(), ctx.logdensity(flat, ignore_prior=False))
    # what the host harness of carma_mband_pt_plan.h draws for the same (seed, chain): the first round whose value is finite
    pr = ctx.prior()
    assert pr == pytest.approx(ptref.prior3(bands), rel=1e-15)
    for k in range(T * Rr):
        for rnd in range(4000):
            cand = pb.draw_start(bands, p, q, pr, lb, SEED, k, rnd)
            if np.isfinite(ctx.logdensity(cand, ignore_prior=False)) and pb.in_box(cand, d, K, box)[0]:
                break
        np.testing.assert_allclose(flat[k], cand, rtol=1e-14, atol=0, err_msg="chain %d, round %d" % (k, rnd))
    # a finite init row becomes every chain of the run; a non-finite one falls back to the draws
    good = flat[3].copy()
    ctx.pt_start(good)
    th2, lp2 = ctx.pt_get_chains()
    assert np.array_equal(th2.reshape(-1, dx), np.tile(good, (T * Rr, 1))) and np.all(lp2 == lp.ravel()[3])
    bad = good.copy()
    bad[d + 1] = box[1][0, 0] + 1.0                          # outside the band box: -inf for the sampler
    for init in (bad, np.where(np.arange(dx) == 1, 5.0, good)):
        ctx.pt_start(init)
        th3, lp3 = ctx.pt_get_chains()
        assert np.array_equal(th3, th) and np.array_equal(lp3, lp)


# ---- 6. recovery -------------------------------------------------------------------------------------------------------------------
# Two runs of 64 replicas.  The COMPARISON run repeats the reference ladder's scheme (burn-in, thinning, length), so that the two
# pooled means estimate the same number whether or not 1000 adapting iterations have converged.  The MAIN run is what a user would
# do -- a burn-in long enough for the factor to settle (the lag's proposal scale starts at the median time step, ~2, and ends near
# 0.03), thinned draws -- and carries the interval, the bit-for-bit checks and the diagnostics.  chain_diag's acor halves a chain
# until tau < 2 and needs 50 rows left: on this problem the lag's autocorrelation time is ~10 iterations once adapted, and
# unthinned chains of 400 ... 16 000 rows from the short burn-in were SHORT in half to three quarters of the ladders.
# acor on a few hundred thinned rows is itself noisy (tau comes out 0.4 ... 4 where ~1 is the truth, and now and then NaN): with
# 500 draws thinned by 16, five seeds left 2, 0, 4, 3, 5 of the 64 ladders SHORT (and the one without had a NaN tau at status 0);
# with 1000 draws 2, 1, 0, 0, 3, and the two seeds without have every value finite (ESS 45 000 of 64 000 draws, R-hat 1.003).
# The run is reproducible from its seed, so the test keeps one of those two.
MAIN_BURN, MAIN_SAMPLES, MAIN_THIN, MAIN_SEED = 4000, 1000, 16, 20240925


def test_run_mcmc_recovers_the_lag_as_the_reference_ladder_does(cpa):
    bands, _ = R.recovery_problem()
    model = cpa.CarmaBandsModel(bands, ptref.RECOVERY_P, ptref.RECOVERY_Q, lag_bounds=ptref.RECOVERY_LAG_BOUNDS)
    nrep, d = 64, 3 + ptref.RECOVERY_P + ptref.RECOVERY_Q
    # -- against the CPU reference ladder (independent seed, the same ladder, burn-in, thinning and length): pooled means, the standard
    # error from the between-ladder scatter of both runs
    c = model.run_mcmc(ptref.RECOVERY_SAMPLES, nburnin=ptref.RECOVERY_BURN, ntemperatures=ptref.RECOVERY_T, nthin=ptref.RECOVERY_THIN,
                       nreplicas=nrep, seed=SEED)
    ref = ptref.recovery_reference()
    m_gpu = c.get_samples("lag").reshape(nrep, ptref.RECOVERY_SAMPLES).mean(axis=1)
    m_ref = ref["samples"][:, :, d].mean(axis=1)
    se = np.sqrt(m_gpu.var(ddof=1) / m_gpu.size + m_ref.var(ddof=1) / m_ref.size)
    print("lag, the reference's scheme: GPU %.4f, reference ladder %.4f, difference %.2f standard errors (se %.4f)"
          % (m_gpu.mean(), m_ref.mean(), (m_gpu.mean() - m_ref.mean()) / se, se))
    assert abs(m_gpu.mean() - m_ref.mean()) <= 4.0 * se
    lo, hi = np.percentile(c.get_samples("lag"), [0.5, 99.5])
    assert lo <= R.RECOVERY_TRUE_LAG <= hi, (lo, hi)
    # -- the main run
    s = model.run_mcmc(MAIN_SAMPLES, nburnin=MAIN_BURN, ntemperatures=ptref.RECOVERY_T, nthin=MAIN_THIN, nreplicas=nrep, seed=MAIN_SEED)
    assert model.mcmc_sample is s
    n = nrep * MAIN_SAMPLES
    lag = s.get_samples("lag")
    assert lag.shape == (n, 1) and np.all(np.isfinite(s.trace))
    lo, hi = np.percentile(lag, [0.5, 99.5])
    print("lag, main run: mean %.4f, central 99 %% [%.4f, %.4f]" % (lag.mean(), lo, hi))
    assert lo <= R.RECOVERY_TRUE_LAG <= hi, (lo, hi)
    assert np.array_equal(s.get_samples("logpost")[:, 0], model.logpost(s.trace))
    assert np.array_equal(s.get_samples("loglik")[:, 0], model.context().logdensity(s.trace, ignore_prior=True))
    diag = s.diagnostics()
    assert diag["tau"].shape == (nrep, model.dx + 1) and diag["ess"].shape == diag["rhat"].shape == (model.dx + 1,)
    print("lag: split R-hat %.4f, ESS %.0f of %d draws, chain_diag status counts %s"
          % (diag["rhat"][d], diag["ess"][d], n, np.bincount(diag["status"][:, d], minlength=4)))
    for k in ("tau", "mean", "sigma"):
        assert np.all(np.isfinite(diag[k][:, d])), (k, np.bincount(diag["status"][:, d], minlength=4))
    assert np.isfinite(diag["ess"][d]) and np.isfinite(diag["rhat"][d])


# ---- 7. the Python API and the C ABI's argument errors -------------------------------------------------------------------------
def test_run_mcmc_shapes_and_smooth_band_at_dx_17(cpa):
    p, q = 5, 3
    bands, extras = R.scenario("three_bands_7_1_12", seed=p)
    model = cpa.CarmaBandsModel(bands, p, q, lag_bounds=[(e[0] - 1.0, e[0] + 1.0) for e in extras])
    assert model.dx == 17
    s = model.run_mcmc(20, nburnin=30, nreplicas=3, seed=5, scale_bounds=[(0.01, 100.0), (0.05, 50.0)])
    n = 60
    assert s.trace.shape == (n, 17) and s.get_samples("lag").shape == (n, 2) and s.get_samples("sigma").shape == (n, 1)
    assert s.get_samples("ar_roots").shape == (n, p) and s.get_samples("ma_coefs").shape == (n, q + 1)
    sc = s.get_samples("scale")
    assert np.all((sc >= [0.01, 0.05]) & (sc <= [100.0, 50.0]))
    med, lo, hi = s.lag_summary()
    assert med.shape == (2,) and np.all(lo <= med) and np.all(med <= hi)
    tt = np.linspace(bands[2][0].min(), bands[2][0].max(), 9)
    for kw in (dict(), dict(nsamples=7), dict(nsamples=7, seed=1)):
        bm, bv = s.smooth_band(tt, band=2, **kw)
        assert bm.shape == bv.shape == (9,) and np.all(np.isfinite(bm)) and np.all(bv > 0)
    lo_psd, hi_psd, mid, f = s.power_spectrum_band(freq=[0.1, 0.5, 1.0])
    assert np.all(np.isfinite(mid)) and np.all(lo_psd <= mid) and np.all(mid <= hi_psd)
    diag = s.diagnostics()
    assert diag["tau"].shape == (3, 18) and diag["rhat"].shape == (18,)


def test_calls_before_create_and_before_start_are_einval(cpa):
    L, EINVAL = cpa._lib.lib, cpa._lib.CARMA_EINVAL
    bands, extras = R.scenario("lag0_shared_stamps", seed=2)
    ctx = cpa.BandsContext(bands, 2, 1, lag_bounds=[(-1.0, 1.0)])
    dp = C.POINTER(C.c_double)
    buf = np.zeros(64 * ctx.dx * ctx.dx)
    p_ = buf.ctypes.data_as(dp)
    before_create = [("set_chains", (p_, None)), ("get_chains", (p_, p_)), ("start", (None,)), ("get_factor", (p_,)),
                     ("set_factor", (p_,)), ("iterate", (1, 1)), ("sample", (1, 1, p_, p_)), ("stats", (p_, p_, 0)), ("logdensity", (p_, p_))]
    for name, args in before_create:
        assert getattr(L, "carma_bands_pt_" + name)(ctx.handle, *args) == EINVAL, name
        assert "call carma_bands_pt_create first" in cpa._lib.last_error(), name
    assert L.carma_bands_pt_iterations_done(ctx.handle) == EINVAL
    assert L.carma_bands_pt_create(ctx.handle, 65, 1, None, 0, 1, None, None) == EINVAL and "64 temperatures" in cpa._lib.last_error()
    lo, hi = np.array([[0.0, 1.0]]), np.array([[1.0, 0.0]])
    assert L.carma_bands_pt_create(ctx.handle, 4, 1, None, 0, 1, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp)) == EINVAL
    assert "lo <= hi" in cpa._lib.last_error()
    ctx.pt_create(4, 2, 5, seed=1, band_box=ctx.pt_default_box())
    for name, args in [("iterate", (1, 1)), ("sample", (1, 1, p_, p_))]:
        assert getattr(L, "carma_bands_pt_" + name)(ctx.handle, *args) == EINVAL, name
        assert "no starting values" in cpa._lib.last_error(), name
    # the context is still usable
    ctx.pt_start()
    ctx.pt_iterate(5)
    sm, sl = ctx.pt_sample(3)
    assert np.array_equal(sl.ravel(), ctx.logdensity(sm.reshape(-1, ctx.dx)))
    ctx.close()
