"""GPU tests of the power-spectrum band of a whole sampled set in one call (carma_mpost.hip: carma_mpsd_band,
_lib.mpsd_band, CarmaModelSet.power_spectrum_band) and of the one sigma launch of CarmaModelSet.run_mcmc.

The yardstick is code from before the set call: the grid that carma_psd_band returns for a series alone with np.percentile
on it (4e-16: numpy's interpolation, the bar of test_gpu_post.test_psd_grid_and_exact_order_statistics), and the reference's
own output in tests/golden/psd.npz (1e-9 / 1e-10, the bars of test_gpu_post.test_psd_band_matches_reference_output)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as orc
from helpers import prior_like_theta

pytestmark = pytest.mark.gpu

PCS = [0.0, 2.5, 50.0, 100.0]
NF_MASTER = 40


@pytest.fixture(scope="module")
def cpa():
    import carma_pack_amd as m
    assert m._lib.lib.carma_device_count() >= 1
    return m


@pytest.fixture(scope="module")
def readme(golden_dir):
    return np.load(os.path.join(golden_dir, "carma53_readme.npz"))


def _derived(cp, th, p, q):
    roots = cp._roots_from_log_quads(th[:, 3:3 + p])
    ar = cp._poly_from_roots(roots).real
    if q:
        c = cp._poly_from_roots(cp._roots_from_log_quads(th[:, 3 + p:3 + p + q]))
        ma = (c / c[:, q:q + 1])[:, ::-1].real
    else:
        ma = np.ones((th.shape[0], 1))
    return roots, ar, ma


def _models(rng, p, q, t, y, nbase):
    """nbase prior-like models of order (p, q): (ar [nbase, p + 1], ma [nbase, q + 1], sigma [nbase])."""
    from carma_pack_amd import carma_pack as cp
    if p == 1:
        ar = np.c_[np.ones(nbase), np.exp(rng.normal(-3.0, 1.0, nbase))]
        return ar, np.ones((nbase, 1)), np.sqrt(2.0 * ar[:, 1] * rng.uniform(0.5, 3.0, nbase) ** 2)
    th = np.array([prior_like_theta(rng, p, q, t, y) for _ in range(nbase)])
    roots, ar, ma = _derived(cp, th, p, q)
    sig = orc.post.sigma_noise(roots, ma, th[:, 0] ** 2)
    sig[~np.isfinite(sig)] = 1.0
    return ar, ma, sig


def _solo(_lib, ar, ma, sig, freq, pcs):
    """What the code before the set call gives for one series: (np.percentile of carma_psd_band's grid [nf, nperc], the grid
    sorted along the samples [nf, ns])."""
    grid = _lib.psd_band(ar, ma, sig, freq, [], return_samples=True)[1]
    with np.errstate(invalid="ignore"):
        return np.percentile(grid, pcs, axis=1).T, np.sort(grid, axis=1)


def _set_call(_lib, series, freqs, pcs, order=None):
    """One mpsd_band call over series (a list of (ar, ma, sig)) in `order`; the band comes back in the list's order."""
    order = list(range(len(series))) if order is None else list(order)
    start = np.r_[0, np.cumsum([series[s][2].size for s in order])]
    band = _lib.mpsd_band(*(np.concatenate([series[s][k] for s in order]) for k in range(3)), start,
                          np.stack([freqs[s] for s in order]), pcs)
    out = np.empty_like(band)
    out[order] = band
    return out


def _check_band(band, want, sorted_grid, pcs, what):
    """band [nf, nperc] of one series against np.percentile of its own grid; where the virtual index is an integer the band
    IS that order statistic of the grid, to the bit."""
    np.testing.assert_allclose(band, want, rtol=4e-16, atol=0.0, err_msg=str(what))
    ns = sorted_grid.shape[1]
    for j, q in enumerate(pcs):
        vi = (ns - 1) * (q / 100.0)
        if vi == np.floor(vi):
            np.testing.assert_array_equal(band[:, j], sorted_grid[:, int(vi)], err_msg="%s, percentile %g" % (what, q))


@pytest.fixture(scope="module")
def ragged(cpa, readme):
    """The ragged CARMA(5,3) set of test 1 with its single-series yardstick on NF_MASTER frequencies, computed once.
    Every series has its own frequency grid; rows have ties (the models are drawn with repeats)."""
    from carma_pack_amd import _lib
    L = _lib.mpsd_fused_max()
    sizes = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, L - 1, L, L + 1, 5003]
    rng = np.random.default_rng(29)
    base = _models(rng, 5, 3, readme["t"], readme["y"], 400)
    master = np.exp(np.linspace(np.log(1e-3), np.log(0.5), NF_MASTER))
    series, freqs, want, sgrid = [], [], [], []
    for s, ns in enumerate(sizes):
        idx = rng.integers(0, min(ns, 400), ns)
        series.append(tuple(a[idx] for a in base))
        freqs.append(master * (1.0 + 0.01 * s))
        w, g = _solo(_lib, *series[-1], freqs[-1], PCS)
        want.append(w)
        sgrid.append(g)
    for a in want + sgrid:
        a.setflags(write=False)
    return dict(sizes=sizes, series=series, freqs=freqs, want=want, sgrid=sgrid)


def _nf_cases():
    from carma_pack_amd import _lib
    ft = _lib.mpsd_freq_tile()
    return sorted({1, 7, 8, 9, 17} | ({ft - 1, ft, ft + 1} if ft != 8 else set()))


def test_exact_selection_ragged_rows_one_call(cpa, ragged):
    """Sample counts either side of a wave, of the workgroup, of the padded row sizes and of the fused limit, in one call;
    then the same series in a shuffled order; at frequency counts either side of 8 and of the kernel's frequency tile."""
    from carma_pack_amd import _lib
    S = len(ragged["sizes"])
    assert NF_MASTER >= max(_nf_cases())
    shuffled = np.random.default_rng(4).permutation(S)
    for nf in _nf_cases():
        freqs = [f[:nf] for f in ragged["freqs"]]
        band = _set_call(_lib, ragged["series"], freqs, PCS)
        assert band.shape == (S, nf, len(PCS))
        for s, ns in enumerate(ragged["sizes"]):
            _check_band(band[s], ragged["want"][s][:nf], ragged["sgrid"][s][:nf], PCS, "ns = %d, nf = %d" % (ns, nf))
        if nf == 17:
            again = _set_call(_lib, ragged["series"], freqs, PCS, order=shuffled)
            np.testing.assert_array_equal(again, band)


@pytest.mark.parametrize("nar", [2, 3, 4, 5, 6, 7, 8])
def test_every_order(cpa, readme, nar):
    """Every (nar, nma) the entry admits, three series of 257, 64 and 300 samples, each with its own nine frequencies cut from
    0 and 16 log-spaced frequencies from 1e-4 to 10."""
    from carma_pack_amd import _lib
    master = np.r_[0.0, np.exp(np.linspace(np.log(1e-4), np.log(10.0), 16))]
    freqs = [master[0:9], master[4:13], master[8:17]]
    pcs = [0.0, 16.0, 50.0, 100.0]
    for nma in range(1, nar):
        rng = np.random.default_rng(100 * nar + nma)
        ar, ma, sig = _models(rng, nar - 1, nma - 1, readme["t"], readme["y"], 300)
        assert ar.shape == (300, nar) and ma.shape == (300, nma)
        series = [(ar[:257], ma[:257], sig[:257]), (ar[100:164], ma[100:164], sig[100:164]), (ar, ma, sig)]
        band = _set_call(_lib, series, freqs, pcs)
        for s in range(3):
            want, sgrid = _solo(_lib, *series[s], freqs[s], pcs)
            _check_band(band[s], want, sgrid, pcs, "nar = %d, nma = %d, series %d" % (nar, nma, s))


def test_special_rows(cpa):
    """Identical samples; infinities (alpha(0) = 0 at f = 0 for 7 of 50 samples) with NaN between two of them, as numpy
    interpolates; a NaN sigma makes its own series NaN and no other."""
    from carma_pack_amd import _lib
    ar = np.tile([1.0, 0.3, 0.02], (50, 1))
    ma, sg = np.ones((50, 1)), np.full(50, 0.7)
    ar0 = ar.copy()
    ar0[:7, 2] = 0.0
    sgn = sg.copy()
    sgn[3] = np.nan
    freq = np.array([0.0, 0.2])
    pcs = [50.0, 100.0, 16.0]
    series = [(ar, ma, sg), (ar0, ma, sg), (ar, ma, sgn)]
    band = _set_call(_lib, series, [freq] * 3, pcs)
    assert np.all(band[0] == band[0][:, :1]) and np.isfinite(band[0]).all()
    want, sgrid = _solo(_lib, *series[1], freq, pcs)
    assert np.isinf(sgrid[0, -7:]).all()
    np.testing.assert_array_equal(band[1], want)
    assert np.isfinite(band[1][0, 0]) and np.isnan(band[1][0, 1]) and np.isfinite(band[1][1]).all()
    assert np.isnan(band[2]).all()
    for s in (0, 1):
        np.testing.assert_array_equal(band[s], _set_call(_lib, [series[s]], [freq], pcs)[0])
    np.testing.assert_array_equal(band[0], _solo(_lib, *series[0], freq, pcs)[0])


def test_independence_and_bounds(cpa, ragged):
    """A series' band does not depend on the set it is in, and a call writes the rows it was asked for and no more."""
    from carma_pack_amd import _lib
    nf = 17
    S = len(ragged["sizes"])
    freqs = [f[:nf] for f in ragged["freqs"]]
    band = _set_call(_lib, ragged["series"], freqs, PCS)
    for s in range(S):
        alone = _set_call(_lib, [ragged["series"][s]], [freqs[s]], PCS)
        np.testing.assert_array_equal(alone[0], band[s], err_msg="ns = %d" % ragged["sizes"][s])
    args = [_lib.as_f64(np.concatenate([x[k] for x in ragged["series"]])) for k in range(3)]
    start = np.r_[0, np.cumsum(ragged["sizes"])].astype(np.int64)
    fr, pc = _lib.as_f64(np.stack(freqs)), _lib.as_f64(PCS)
    buf = np.full((S + 1, nf, len(PCS)), -777.0)
    rc = _lib.lib.carma_mpsd_band(6, 4, _lib.ptr(args[0]), _lib.ptr(args[1]), _lib.ptr(args[2]),
                                  start.ctypes.data_as(C.POINTER(C.c_long)), S, _lib.ptr(fr), nf, _lib.ptr(pc), len(PCS),
                                  _lib.ptr(buf), _lib.default_device())
    assert rc == 0
    assert (buf[S] == -777.0).all()
    np.testing.assert_array_equal(buf[:S], band)


def test_reference_output(cpa, readme, golden_dir):
    """The reference's own plot_power_spectrum numbers (tests/golden/psd.npz) on its frequency grids: the 32 README vectors
    in full and subsampled to 9 as two series of one set, and the CAR(1) vectors in a call of their own."""
    from carma_pack_amd import _lib, carma_pack as cp
    ref = np.load(os.path.join(golden_dir, "psd.npz"))
    th = readme["theta"]
    roots, ar, ma = _derived(cp, th, 5, 3)
    sig = _lib.sigma_noise_batch(roots, ma, th[:, 0] ** 2)
    idx = cp.CarmaSample._subsample(9, th.shape[0])
    series = [(ar, ma, sig), (ar[idx], ma[idx], sig[idx])]
    freqs = [ref["freq"], ref["freq"]]
    b68 = _set_call(_lib, series, freqs, [16.0, 50.0, 84.0])
    b95 = _set_call(_lib, series, freqs, [2.5, 50.0, 97.5])
    for j, key in enumerate(("lo68", "med68", "hi68")):
        np.testing.assert_allclose(b68[0][:, j], ref[key], rtol=1e-9)
    for j, key in enumerate(("lo95_n9", "med95_n9", "hi95_n9")):
        np.testing.assert_allclose(b95[1][:, j], ref[key], rtol=1e-9)
    c1 = ref["car1_theta"]
    om = np.exp(c1[:, 3])
    car1 = (np.c_[np.ones_like(om), om], np.ones((om.size, 1)), np.sqrt(2.0 * om * c1[:, 0] ** 2))
    b1 = _set_call(_lib, [car1], [ref["car1_freq"]], [16.0, 50.0, 84.0])
    for j, key in enumerate(("car1_lo68", "car1_med68", "car1_hi68")):
        np.testing.assert_allclose(b1[0][:, j], ref[key], rtol=1e-10)


def _check_set_api(mset, samples):
    for kw in (dict(percentile=68.0), dict(percentile=95.0, nsamples=57)):
        lo, hi, med, f = mset.power_spectrum_band(**kw)
        assert lo.shape == hi.shape == med.shape == f.shape == (mset.nseries, 1000)
        for s, smp in enumerate(samples):
            lo1, hi1, med1, f1 = smp.power_spectrum_band(**kw)
            np.testing.assert_array_equal(f[s], f1)
            for got, want in ((lo[s], lo1), (hi[s], hi1), (med[s], med1)):
                np.testing.assert_allclose(got, want, rtol=4e-16, atol=0.0, err_msg="series %d, %r" % (s, kw))
    # a caller's grid, for all series and per series; the samples handed over by name
    grid = np.exp(np.linspace(np.log(1e-3), np.log(1.0), 13))
    lo, hi, med, f = mset.power_spectrum_band(68.0, freq=grid, samples=samples)
    lo2, hi2, med2, f2 = mset.power_spectrum_band(68.0, freq=np.tile(grid, (mset.nseries, 1)))
    for a, b in ((lo, lo2), (hi, hi2), (med, med2), (f, f2)):
        np.testing.assert_array_equal(a, b)
    for s, smp in enumerate(samples):
        np.testing.assert_allclose(med[s], smp.power_spectrum_band(68.0, freq=grid)[2], rtol=4e-16, atol=0.0)


def test_api_set_band_and_sigma_of_a_set_run(cpa, readme):
    """CarmaModelSet.run_mcmc then power_spectrum_band: every series' band equals its own CarmaSample's, and the "sigma"
    column that run_mcmc computed for all series in one launch equals the launch of each series on its own, bit for bit."""
    from carma_pack_amd import _lib
    t, y, yerr = readme["t"], readme["y"], readme["yerr"]
    cuts = [60, 110, 165, 220, 270]
    mset = cpa.CarmaModelSet([(t[:n], y[:n], yerr[:n]) for n in cuts], p=5, q=3)
    samples = mset.run_mcmc(120, nburnin=60, ntemperatures=4, seed=3)
    assert len(samples) == 5 and mset.mcmc_samples is samples
    for smp in samples:
        sigma = np.ravel(smp.get_samples("sigma"))
        assert sigma.shape == (120,)
        want = _lib.sigma_noise_batch(smp.get_samples("ar_roots"), smp.get_samples("ma_coefs"), np.ravel(smp.get_samples("var")))
        np.testing.assert_array_equal(sigma, want)
        assert smp._sampler.getSigmaNoise(smp.get_samples("ar_roots"), smp.get_samples("ma_coefs"),
                                          np.ravel(smp.get_samples("var"))) is not None
    _check_set_api(mset, samples)


def test_api_car1_set(cpa, readme):
    """The same for a CAR(1) set of three series (Car1Sample computes its sigma = sqrt(2 omega var) on the host)."""
    t, y, yerr = readme["t"], readme["y"], readme["yerr"]
    mset = cpa.CarmaModelSet([(t[:n], y[:n], yerr[:n]) for n in (80, 150, 270)], p=1)
    samples = mset.run_mcmc(120, nburnin=60, seed=3)
    for smp in samples:
        om = np.exp(np.ravel(smp.get_samples("log_omega")))
        np.testing.assert_array_equal(np.ravel(smp.get_samples("sigma")), np.sqrt(2.0 * om * np.ravel(smp.get_samples("var"))))
    _check_set_api(mset, samples)
