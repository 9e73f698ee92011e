"""The host side of the bands sampler, without a GPU: carma_mband_pt_plan.h (initial factor, starting draws, default box, argument
errors), the RAM-kernel planner of carma_shape_plan.h, the reference ladder (carma_pt_core.h at any dimension) on the lag-recovery
problem, and CarmaBandsSample / the argument checks of CarmaBandsModel.run_mcmc."""
import numpy as np
import pytest

import mband_pt_build as pb
import mband_pt_ref as ptref
import mband_ref as R


# ---- carma_mband_pt_plan.h ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,p,q", [("lag0_shared_stamps", 2, 1), ("three_bands_7_1_12", 5, 3), ("eight_bands", 7, 6)])
def test_initial_factor_entries(name, p, q):
    bands = pb.prepared(R.scenario(name, seed=p)[0])
    K, d = len(bands), 3 + p + q
    R0 = pb.initial_factor(bands, d)
    dx = d + 3 * (K - 1)
    assert R0.shape == (dx, dx) and np.array_equal(R0, np.diag(np.diag(R0)))
    t0, y0, _ = bands[0]
    var0 = np.mean(y0 * y0) - np.mean(y0) ** 2
    want = np.full(dx, 0.01)
    want[0], want[2] = np.sqrt(2.0 * var0 * var0 / y0.size), np.sqrt(var0 / y0.size)
    for b in range(1, K):
        yb = bands[b][1]
        c = d + 3 * (b - 1)
        want[c] = np.median(np.diff(t0))
        want[c + 2] = np.sqrt((np.mean(yb * yb) - np.mean(yb) ** 2) / yb.size) if yb.size >= 2 else 0.01
    np.testing.assert_allclose(np.diag(R0), want, rtol=1e-12)
    assert np.all(np.diag(R0) > 0)
    if name == "three_bands_7_1_12":
        assert R0[d + 2, d + 2] == 0.01                      # the band of one datum


def test_start_draws_are_reproducible_and_inside_the_lag_boxes():
    bands = pb.prepared(R.scenario("eight_bands", seed=2)[0])
    p, q, K = 2, 1, 8
    d = 3 + p + q
    pr = ptref.prior3(bands)
    lb = np.array([(-1.0 - 0.1 * b, 0.5 + 0.2 * b) for b in range(K - 1)])
    cols = d + 3 * np.arange(K - 1)
    seen = []
    for seed, chain, rnd in [(7, 0, 0), (7, 1, 0), (7, 0, 1), (8, 0, 0), (7, 63, 5)]:
        a = pb.draw_start(bands, p, q, pr, lb, seed, chain, rnd)
        assert np.array_equal(a, pb.draw_start(bands, p, q, pr, lb, seed, chain, rnd))
        assert np.all(np.isfinite(a))
        assert np.all((a[cols] >= lb[:, 0]) & (a[cols] <= lb[:, 1]))
        s0 = bands[0][1].std(ddof=1)
        for b in range(1, K):
            yb = bands[b][1]
            assert a[cols[b - 1] + 1] == pytest.approx(np.log(yb.std(ddof=1) / s0), rel=1e-12)
            assert a[cols[b - 1] + 2] == pytest.approx(yb.mean(), rel=1e-12)
        seen.append(a)
    for i in range(len(seen)):
        for j in range(i):
            assert not np.array_equal(seen[i][:d + 1], seen[j][:d + 1])   # (seed, chain, round) each move the draw


def test_start_of_a_one_datum_band_and_the_default_box():
    bands = pb.prepared(R.scenario("three_bands_7_1_12", seed=5)[0])
    d = 3 + 5 + 3
    a = pb.draw_start(bands, 5, 3, ptref.prior3(bands), [(-2, 2), (-3, 3)], 1, 0, 0)
    assert a[d + 1] == 0.0 and a[d + 2] == bands[1][1][0]    # log a undefined -> 0; mu = the datum
    lo, hi = pb.default_box(bands)
    assert lo.shape == hi.shape == (2, 2)
    y1, y2 = bands[1][1], bands[2][1]
    np.testing.assert_allclose([lo[0, 0], hi[0, 0]], [-np.log(1000.0), np.log(1000.0)], rtol=1e-12)
    span1 = max(1.0, abs(y1[0]))                             # one datum: no span of its own
    np.testing.assert_allclose([lo[0, 1], hi[0, 1]], [y1[0] - span1, y1[0] + span1], rtol=1e-12)
    la = np.log(y2.std(ddof=1) / bands[0][1].std(ddof=1))
    np.testing.assert_allclose([lo[1, 0], hi[1, 0]], [la - np.log(1000.0), la + np.log(1000.0)], rtol=1e-12)
    span2 = y2.max() - y2.min()
    np.testing.assert_allclose([lo[1, 1], hi[1, 1]], [y2.min() - span2, y2.max() + span2], rtol=1e-12)
    # a start lies inside the default box; in_box of the header agrees with the numpy statement of it
    assert pb.in_box(a, d, 3, (lo, hi))[0]
    L = pb.plan()
    for row, want in [(a, 1), (np.where(np.arange(a.size) == d + 1, hi[0, 0] + 1e-9, a), 0),
                      (np.where(np.arange(a.size) == d + 5, lo[1, 1] - 1e-9, a), 0), (np.where(np.arange(a.size) == d + 2, np.nan, a), 0)]:
        row = np.ascontiguousarray(row)
        assert L.mbpt_in_box(pb._p(row), d, 3, pb._p(np.ascontiguousarray(lo)), pb._p(np.ascontiguousarray(hi))) == want
        assert bool(pb.in_box(row, d, 3, (lo, hi))[0]) == bool(want)
    assert L.mbpt_in_box(pb._p(np.ascontiguousarray(a)), d, 3, None, None) == 1   # a null box is no box


def test_create_argument_errors_carry_messages():
    ok = dict(ntemps=10, nreplicas=2, adapt_iters=5, dx=9, K=2)
    assert pb.check_create(**ok) == ""
    assert pb.check_create(**dict(ok, ntemps=64)) == "" and pb.check_create(**dict(ok, ntemps=1)) == ""
    for bad in (0, 65, -3):
        assert "1 ... 64 temperatures" in pb.check_create(**dict(ok, ntemps=bad))
    assert "nreplicas < 1" in pb.check_create(**dict(ok, nreplicas=0))
    assert "adapt_iters < 0" in pb.check_create(**dict(ok, adapt_iters=-1))
    assert "more than one launch can index" in pb.check_create(**dict(ok, ntemps=64, nreplicas=2 ** 26))
    assert pb.check_create(**dict(ok, dx=37, K=8)) == ""
    assert "37 at most" in pb.check_create(**dict(ok, dx=38, K=8))
    assert "band 0 needs at least 2 data" in pb.check_create(n0=1, **ok)
    lo, hi = np.array([[-1.0, 0.0]]), np.array([[1.0, 2.0]])
    assert pb.check_create(band_lo=lo, band_hi=hi, **ok) == ""
    assert pb.check_create(band_lo=lo, band_hi=lo, **ok) == ""            # lo == hi is legal
    assert "come together" in pb.check_create(band_lo=lo, **ok)
    msg = pb.check_create(band_lo=np.array([[-1.0, 3.0]]), band_hi=hi, **ok)
    assert "band 1, mu" in msg and "lo <= hi" in msg
    assert "band 1, log a" in pb.check_create(band_lo=np.array([[np.nan, 0.0]]), band_hi=hi, **ok)


def test_chunk_sizing_follows_the_total_number_of_data():
    L = pb.plan()
    assert L.mbpt_chunk_iters(1) == 4096 and L.mbpt_chunk_iters(28) == 4096
    assert L.mbpt_chunk_iters(1000) == int(250000.0 / 450.0) and L.mbpt_chunk_iters(10 ** 7) == 1


# ---- which RAM bookkeeping serves a dimension (carma_shape_plan.h) ------------------------------------------------------------------
def test_ram_kernel_planner():
    assert [pb.ram_kernels_plan(d) for d in (4, 12, 13, 16, 17, 37)] == \
        [pb.RAM_FUSED, pb.RAM_FUSED, pb.RAM_SPLIT, pb.RAM_SPLIT, pb.RAM_WIDE, pb.RAM_WIDE]
    assert [pb.ram_kernels_plan(d, 4) for d in (4, 12, 13, 16, 17, 37)] == [pb.RAM_WIDE] * 6
    assert [pb.ram_kernels_plan(d, 13) for d in (4, 12, 13, 16, 17)] == [pb.RAM_FUSED, pb.RAM_FUSED, pb.RAM_WIDE, pb.RAM_WIDE, pb.RAM_WIDE]
    assert pb.ram_kernels_plan(17, 30) == pb.RAM_WIDE        # no templated kernel exists beyond 16, whatever the entry says
    assert [pb.ram_kernels_plan(d) for d in (0, 3, 38, 100)] == [pb.RAM_NONE] * 4
    assert pb.ram_kernels_plan(3, 4) == pb.RAM_NONE and pb.ram_kernels_plan(38, 4) == pb.RAM_NONE


# ---- the reference ladder on the recovery problem -------------------------------------------------------------------------------
def test_reference_ladder_recovers_the_lag():
    ref = ptref.recovery_reference()
    lad, samples = ref["ladder"], ref["samples"]
    d = 3 + ptref.RECOVERY_P + ptref.RECOVERY_Q
    assert samples.shape == (ptref.RECOVERY_LADDERS, ptref.RECOVERY_SAMPLES, d + 3)
    assert np.all(np.isfinite(lad.theta)) and np.all(np.isfinite(lad.lp)) and np.all(np.isfinite(lad.chol))
    assert np.all(np.isfinite(samples)) and np.all(np.isfinite(ref["logposts"]))
    lag = samples[:, :, d]
    assert np.all((lag >= 0.0) & (lag <= 8.0))
    assert pb.in_box(samples.reshape(-1, d + 3), d, 2, ref["box"]).all()
    lo, hi = np.percentile(lag, [0.5, 99.5])
    print("reference ladder: lag mean %.4f, central 99 %% [%.4f, %.4f], cold accept rate %.3f"
          % (lag.mean(), lo, hi, lad.nacc[:, 0].mean() / lad.iter))
    assert lo <= R.RECOVERY_TRUE_LAG <= hi
    # the saved log-posteriors are the log-density of the saved values
    np.testing.assert_array_equal(ref["dens"](samples.reshape(-1, d + 3)), ref["logposts"].ravel())


def test_reference_ladder_is_reproducible_from_its_seed():
    ref = ptref.recovery_reference()
    theta, lp = ref["start"]
    T, d = ptref.RECOVERY_T, 3 + ptref.RECOVERY_P + ptref.RECOVERY_Q + 3
    bands, _ = R.recovery_problem()
    R0 = pb.initial_factor(bands, d - 3)

    def run(seed, parts):
        lad = pb.Ladder(ref["dens"], d, T, 2, 12, seed, theta[:2 * T], lp[:2 * T], np.tile(R0, (2 * T, 1, 1)))
        for n in parts:
            lad.iterate(n)
        s, l = lad.sample(4, 2)
        return lad.theta, lad.lp, lad.chol, lad.nacc, lad.nswap, s, l

    a, b, c = run(11, [20]), run(11, [7, 13]), run(12, [20])
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert not np.array_equal(a[0], c[0])
    assert not np.array_equal(a[0][0], a[0][1])              # the two ladders differ


# ---- CarmaBandsSample and run_mcmc's argument checks, without a device ----------------------------------------------------------
def _synthetic_sample(K=3, p=3, q=1, R_=2, n=40):
    import carma_pack_amd as cpa
    from carma_pack_amd.carma_pack import carma_variance
    rng = np.random.default_rng(5)
    bands = [(np.sort(rng.uniform(0, 50, 15 + b)), rng.standard_normal(15 + b), np.full(15 + b, 0.1)) for b in range(K)]
    model = cpa.CarmaBandsModel(bands, p, q, lag_bounds=[(-3, 3)] * (K - 1))
    th = R.order_thetas(p, q)[0]
    samples = np.tile(np.concatenate([th, np.tile([0.5, 0.1, 1.0], K - 1)]), (R_, n, 1)) + 0.01 * rng.standard_normal((R_, n, model.dx))
    logposts = rng.standard_normal((R_, n))
    loglik = rng.standard_normal(R_ * n)
    tr = samples.reshape(-1, model.dx)
    roots, ma, var = cpa.CarmaSample._sigma_inputs_of(tr[:, :model.d], p, q)
    sigma = np.array([np.sqrt(v / carma_variance(1.0, r, m)) for r, m, v in zip(roots, ma, var)])
    return model, samples, logposts, loglik, cpa.CarmaBandsSample(model, samples, logposts, loglik=loglik, sigma=sigma)


def test_bands_sample_entries_and_lag_summary():
    model, samples, logposts, loglik, s = _synthetic_sample()
    n, K, p, q = samples.shape[0] * samples.shape[1], 3, 3, 1
    shapes = dict(var=(n, 1), measerr_scale=(n, 1), mu=(n, 1), quad_coefs=(n, p), ar_roots=(n, p), psd_centroid=(n, p),
                  psd_width=(n, p), ar_coefs=(n, p + 1), ma_coefs=(n, q + 1), sigma=(n, 1), lag=(n, K - 1), log_scale=(n, K - 1),
                  scale=(n, K - 1), offset=(n, K - 1), logpost=(n, 1), loglik=(n, 1))
    assert sorted(s.parameters) == sorted(shapes)
    for k, shp in shapes.items():
        assert s.get_samples(k).shape == shp, k
    tr = samples.reshape(n, -1)
    cols = model.d + 3 * np.arange(K - 1)
    np.testing.assert_array_equal(s.get_samples("lag"), tr[:, cols])
    np.testing.assert_array_equal(s.get_samples("scale"), np.exp(tr[:, cols + 1]))
    np.testing.assert_array_equal(s.get_samples("offset"), tr[:, cols + 2])
    np.testing.assert_array_equal(s.get_samples("logpost")[:, 0], logposts.ravel())      # replica after replica
    np.testing.assert_array_equal(s.get_samples("loglik")[:, 0], loglik)
    np.testing.assert_array_equal(s.get_samples("var")[:, 0], tr[:, 0] ** 2)
    for pc in (68.0, 95.0):
        med, lo, hi = s.lag_summary(pc)
        want = np.percentile(tr[:, cols], [50.0, (100 - pc) / 2, 100 - (100 - pc) / 2], axis=0)
        assert med.shape == lo.shape == hi.shape == (K - 1,)
        np.testing.assert_array_equal(np.array([med, lo, hi]), want)
    assert not hasattr(s, "predict") and not hasattr(s, "simulate")
    with pytest.raises(ValueError):
        type(s)(model, samples[:, :, :-1], logposts)


def test_run_mcmc_argument_errors_come_before_any_device_call():
    model = _synthetic_sample()[0]
    model.context = lambda: pytest.fail("run_mcmc touched the device before its argument checks")
    with pytest.raises(ValueError, match="nsamples"):
        model.run_mcmc(0)
    with pytest.raises(ValueError, match="init"):
        model.run_mcmc(10, init=np.zeros(model.dx - 1))
    with pytest.raises(ValueError, match="init"):
        model.run_mcmc(10, init=np.zeros((2, model.dx)))
    with pytest.raises(ValueError, match="scale_bounds"):
        model.run_mcmc(10, scale_bounds=[(0.1, 10.0)])
    with pytest.raises(ValueError, match="scale_bounds"):
        model.run_mcmc(10, scale_bounds=[(0.1, 10.0), (2.0, 1.0)])
    with pytest.raises(ValueError, match="scale_bounds"):
        model.run_mcmc(10, scale_bounds=[(0.0, 10.0), (1.0, 2.0)])
    with pytest.raises(ValueError, match="offset_bounds"):
        model.run_mcmc(10, offset_bounds=[(0.0, 1.0, 2.0)] * 2)
    model.K = 0
    with pytest.raises(ValueError, match="at least one band"):
        model.run_mcmc(10)
