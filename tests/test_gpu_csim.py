"""GPU tests of the conditional simulation of many paths, a model each (carma_simulate_cond_carma / _car1, k_csim_paths_* and
k_csim_predict_*) and of the Python API on top of it (simulate_cond_*, SimulateBatch, simulate_paths).

The main test is exact: the two kernels reuse simulate_run and predict_run, and the three sums they add are rounded one by
one, so every path is rebuilt BIT FOR BIT from carma_simulate_*, numpy and carma_predict_*."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20240611


@pytest.fixture(scope="module")
def lib():
    import carma_pack_amd._lib as L
    assert L.lib.carma_device_count() >= 1
    return L


def _series(n, seed):
    rng = np.random.RandomState(seed)
    t = np.cumsum(rng.uniform(0.3, 2.0, size=n))
    y = 10.0 + np.cumsum(rng.standard_normal(n)) * 0.3
    yerr = rng.uniform(0.05, 0.3, size=n)
    return t, y, yerr


def _models(p, q, K, seed):
    """K distinct stationary CARMA(p,q) models: (sigsqr [K], roots [K][p], ma [K][q+1], mu [K]); mu[1] = 0 where there is a
    path 1 (the sum that adds mu back is skipped for it), and model 0 hands its roots over real root first."""
    rng = np.random.RandomState(seed)
    roots = np.empty((K, p), dtype=complex)
    for k in range(K):
        r = []
        for _ in range(p // 2):
            a, b = rng.uniform(0.05, 0.6), rng.uniform(0.2, 2.0)
            r += [-a - 1j * b, -a + 1j * b]
        if p % 2:
            r.append(-rng.uniform(0.02, 0.5) + 0j)
        if p == 2 and k == K - 1:
            r = [-0.15 + 0j, -0.9 + 0j]                       # two real roots
        roots[k] = r[::-1] if k == 0 else r
    ma = np.c_[np.ones(K), rng.uniform(0.2, 3.0, size=(K, q))]
    sigsqr = rng.uniform(0.05, 0.5, size=K)
    mu = rng.uniform(8.0, 12.0, size=K)
    if K > 1:
        mu[1] = 0.0
    return sigsqr, roots, ma, mu


def _tsim(t, M):
    """Unsorted: a forecast, a backcast, a time equal to a datum, interior times and one duplicated value."""
    mid = 0.5 * (t[0] + t[1])
    full = np.array([t[-1] + 3.7, t[0] - 2.5, t[min(17, t.size - 1)], mid, t[-1] - 0.01, mid, t[0] + 0.013])
    return full[:M]


def _add_back(x, mu):
    return x + mu if mu != 0.0 else x


def _cond(lib, p, t, y, yerr, sig, roots, ma, mu, ts, **kw):
    if p == 1:
        return lib.simulate_cond_car1(t, y, yerr, sig, -roots[:, 0].real, mu, ts, **kw)
    return lib.simulate_cond_carma(t, y, yerr, sig, roots, ma, mu, ts, **kw)


def _rebuild(lib, p, t, y, yerr, sig, roots, ma, mu, ts, seed, path, unc, noise):
    """Path `path` of model (sig, roots, ma, mu) from the single-model entry points and numpy."""
    grid, dpos, spos = lib.merged_times(t, ts)
    if p == 1:
        f = lib.simulate_car1(grid, sig, -roots[0].real, npaths=path + 1, seed=seed)[path]
    else:
        f = lib.simulate_carma(grid, sig, roots, ma, npaths=path + 1, seed=seed)[path]
    resid = (y - mu) - (unc[dpos] + yerr * noise)             # every operation rounded on its own, as the kernel does
    if p == 1:
        pm = lib.predict_car1(t, resid, yerr, sig, -roots[0].real, ts)[0]
    else:
        pm = lib.predict_carma(t, resid, yerr, sig, roots, ma, ts)[0]
    return f, _add_back(unc[spos] + pm, mu)


@pytest.mark.parametrize("K,M,n", [(5, 7, 40), (1, 1, 2)])
@pytest.mark.parametrize("p,q", [(1, 0), (2, 0), (5, 3), (7, 6)])
def test_every_path_is_the_composition_of_simulate_and_predict(lib, p, q, K, M, n):
    """35 (path, time) pairs: the last wave is partial and waves span two paths; and the smallest call there is."""
    t, y, yerr = _series(n, 3)
    sig, roots, ma, mu = _models(p, q, K, 10 * p + q)
    ts = _tsim(t, M)
    path0 = 3
    out, unc, noise, grid = _cond(lib, p, t, y, yerr, sig, roots, ma, mu, ts, seed=SEED, path0=path0, return_parts=True)
    assert out.shape == (K, M) and unc.shape == (K, n + M) and noise.shape == (K, n)
    assert np.array_equal(grid, lib.merged_times(t, ts)[0]) and np.all(np.diff(grid) >= 0)
    assert np.all(np.isfinite(noise)) and np.all(np.isfinite(out))
    if K > 1:
        assert len({noise[k, 0] for k in range(K)}) == K      # a key per path
    again = _cond(lib, p, t, y, yerr, sig, roots, ma, mu, ts, seed=SEED, path0=path0, return_parts=True)
    assert np.array_equal(again[2], noise) and np.array_equal(again[0], out)
    for k in range(K):
        f, want = _rebuild(lib, p, t, y, yerr, sig[k], roots[k], ma[k], mu[k], ts, SEED, path0 + k, unc[k], noise[k])
        assert np.array_equal(unc[k], f), (k, np.max(np.abs(unc[k] - f)))
        assert np.array_equal(out[k], want), (k, out[k] - want)
    # without the optional outputs: same bits
    assert np.array_equal(_cond(lib, p, t, y, yerr, sig, roots, ma, mu, ts, seed=SEED, path0=path0), out)
    if M > 1:                                                 # the duplicated time and the time equal to a datum
        assert ts[3] == ts[5] and abs(out[0, 3] - out[0, 5]) <= 1e-9 * max(1.0, abs(out[0, 3]))
        assert ts[2] in t


def test_unsorted_series_with_repeated_times_is_prepared_as_the_filter_prepares_it(lib):
    t, y, yerr = _series(12, 4)
    sig, roots, ma, mu = _models(3, 1, 2, 5)
    ts = _tsim(t, 4)
    want = lib.simulate_cond_carma(t, y, yerr, sig, roots, ma, mu, ts, seed=1, return_parts=True)
    perm = np.r_[np.random.RandomState(0).permutation(12), 4]            # shuffled, datum 4 once more behind the others
    y2 = y[perm].copy()
    y2[-1] += 5.0                                                        # (the later duplicate is the one dropped)
    got = lib.simulate_cond_carma(t[perm], y2, yerr[perm], sig, roots, ma, mu, ts, seed=1, return_parts=True)
    for a, b in zip(want, got):
        assert a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("p,q", [(1, 0), (5, 3)])
def test_a_path_does_not_depend_on_its_batch(lib, p, q):
    t, y, yerr = _series(40, 3)
    sig, roots, ma, mu = _models(p, q, 5, 77)
    ts = _tsim(t, 7)
    full = _cond(lib, p, t, y, yerr, sig, roots, ma, mu, ts, seed=SEED)
    a = _cond(lib, p, t, y, yerr, sig[:2], roots[:2], ma[:2], mu[:2], ts, seed=SEED, path0=0)
    b = _cond(lib, p, t, y, yerr, sig[2:], roots[2:], ma[2:], mu[2:], ts, seed=SEED, path0=2)
    assert np.array_equal(np.vstack([a, b]), full)
    try:
        lib.tune_set("CSIM_CHUNK_PATHS", 3)                              # chunks of 3 + 2 paths
        chunked = _cond(lib, p, t, y, yerr, sig, roots, ma, mu, ts, seed=SEED, return_parts=True)
    finally:
        lib.tune_set("CSIM_CHUNK_PATHS", None)
    whole = _cond(lib, p, t, y, yerr, sig, roots, ma, mu, ts, seed=SEED, return_parts=True)
    for c, w in zip(chunked, whole):
        assert np.array_equal(c, w)
    assert np.array_equal(whole[0], full)
    assert not np.array_equal(_cond(lib, p, t, y, yerr, sig, roots, ma, mu, ts, seed=SEED + 1), full)


@pytest.fixture(scope="module")
def dense(golden_dir):
    """Dense-GP conditional mean / Cholesky factor of the process at 6 times given 30 data, for the p = 5 model of
    cpp_carma_test300.npz (as the file holds it: five MA coefficients) and one CAR(1) model (computed once; built as
    test_simulate_is_a_draw_from_the_dense_gp_conditional builds it)."""
    import oracle as orc
    res = {}
    g = np.load(os.path.join(golden_dir, "cpp_carma_test300.npz"))
    c = np.load(os.path.join(golden_dir, "car1_n100.npz"))
    th = c["theta"][0]
    om1 = float(np.exp(th[3]))
    cases = {5: (g["t"][:30], g["y"][:30], g["yerr"][:30], float(g["sigsqr"]), g["omega"], g["ma"]),
             1: (c["t"][:30], c["y"][:30], c["yerr"][:30], 2.0 * om1 * th[0] ** 2, np.array([-om1 + 0j]), np.ones(1))}
    for p, (t, y, e, sigsqr, roots, ma) in cases.items():
        span = t[-1] - t[0]
        ts = np.r_[t[0] - 0.05 * span, 0.5 * (t[4] + t[5]), t[12] + 0.3 * (t[13] - t[12]), 0.5 * (t[20] + t[21]),
                   t[27] + 0.7 * (t[28] - t[27]), t[-1] + 0.05 * span]
        ns = ts.size
        tc = np.concatenate([ts, t])
        lags, inv = np.unique(np.abs(tc[:, None] - tc[None, :]).ravel(), return_inverse=True)
        acv = np.array([orc.variance(roots, ma, np.sqrt(sigsqr), float(dt)) for dt in lags])
        cov = acv[inv].reshape(tc.size, tc.size)
        cov[np.arange(ns, tc.size), np.arange(ns, tc.size)] += e * e
        Kdd, Ksd, Kss = cov[ns:, ns:], cov[:ns, ns:], cov[:ns, :ns]
        sol = np.linalg.solve(Kdd, np.c_[y, Ksd.T])
        cmean, cvar = Ksd @ sol[:, 0], Kss - Ksd @ sol[:, 1:]
        res[p] = dict(t=t, y=y, e=e, sigsqr=sigsqr, roots=roots, ma=ma, ts=ts, cmean=cmean,
                      L=np.linalg.cholesky(0.5 * (cvar + cvar.T)))
    return res


@pytest.mark.parametrize("p", [1, 5])
def test_the_ensemble_is_the_dense_gp_conditional(lib, dense, p):
    """2048 paths of one model, whitened by the dense conditional: mean 0, covariance 1, every entry within 5 sigma of its
    sampling error (a correct sampler fails about once in 1e6 per entry).  A wrong key pairing, missing noise or the wrong
    sign of the residual breaks these by orders of magnitude."""
    d = dense[p]
    K, M = 2048, d["ts"].size
    sig, roots, ma = np.full(K, d["sigsqr"]), np.tile(d["roots"], (K, 1)), np.tile(d["ma"], (K, 1))
    out = _cond(lib, p, d["t"], d["y"], d["e"], sig, roots, ma, None, d["ts"], seed=SEED)
    assert out.shape == (K, M) and np.all(np.isfinite(out))
    z = np.linalg.solve(d["L"], (out - d["cmean"]).T).T
    zm = z.mean(axis=0)
    zc = (z - zm).T @ (z - zm) / (K - 1)
    print("whitened mean", zm, "\nwhitened covariance\n", zc)
    assert np.all(np.abs(zm) <= 5.0 / np.sqrt(K)), zm
    off = zc - np.diag(np.diag(zc))
    assert np.all(np.abs(off) <= 5.0 / np.sqrt(K)), off
    assert np.all(np.abs(np.diag(zc) - 1.0) <= 5.0 * np.sqrt(2.0 / K)), np.diag(zc)
    if p == 1:
        pm, pv = lib.predict_car1(d["t"], d["y"], d["e"], d["sigsqr"], -d["roots"][0].real, d["ts"])
    else:
        pm, pv = lib.predict_carma(d["t"], d["y"], d["e"], d["sigsqr"], d["roots"], d["ma"], d["ts"])
    print("ensemble mean - predict mean, in sigma", (out.mean(axis=0) - pm) / np.sqrt(pv / K))
    assert np.all(np.abs(out.mean(axis=0) - pm) <= 5.0 * np.sqrt(pv / K))


def test_a_singular_path_flags_itself_only(lib):
    t, y, yerr = _series(40, 3)
    sig, roots, ma, mu = _models(3, 1, 5, 9)
    ts = _tsim(t, 7)
    good = lib.simulate_cond_carma(t, y, yerr, sig, roots, ma, mu, ts, seed=SEED, return_singular=True)
    assert not good[1].any()
    bad = roots.copy()
    bad[2] = [-0.5, -0.5, -0.2]                                          # a repeated AR root
    out, flags = lib.simulate_cond_carma(t, y, yerr, sig, bad, ma, mu, ts, seed=SEED, return_singular=True)
    assert flags.tolist() == [False, False, True, False, False]
    keep = [0, 1, 3, 4]
    assert np.array_equal(out[keep], good[0][keep])
    with pytest.raises(lib.CarmaError, match="path 2"):
        lib.simulate_cond_carma(t, y, yerr, sig, bad, ma, mu, ts, seed=SEED)
    # the C entry point without a flag array: 1
    import ctypes as C
    om = np.ascontiguousarray(np.stack([bad.real, bad.imag], axis=-1))
    o = np.empty((5, 7))
    rc = lib.lib.carma_simulate_cond_carma(lib.ptr(t), lib.ptr(y), lib.ptr(yerr), t.size, 3, 5, lib.ptr(sig), lib.ptr(om),
                                           lib.ptr(np.ascontiguousarray(ma)), 2, lib.ptr(mu), lib.ptr(ts), 7, C.c_uint64(SEED), 0,
                                           lib.ptr(o), None, None, None, None, lib.default_device())
    assert rc == 1 and np.array_equal(o[keep], good[0][keep])


@pytest.fixture(scope="module")
def samples(golden_dir):
    import carmcmc as cm
    g = np.load(os.path.join(golden_dir, "carma53_readme.npz"))
    t, y, e = g["t"][:60], g["y"][:60], g["yerr"][:60]
    s31 = cm.CarmaModel(t, y, e, p=3, q=1).run_mcmc(200, nburnin=100, seed=5)
    s1 = cm.CarmaModel(t, y, e, p=1).run_mcmc(200, nburnin=100, seed=5)
    assert isinstance(s1, cm.Car1Sample) and not isinstance(s31, cm.Car1Sample)
    return cm, t, y, e, {3: s31, 1: s1}


@pytest.mark.parametrize("p", [3, 1])
def test_simulate_paths_and_simulate_batch(lib, samples, p):
    cm, t, y, e, ss = samples
    sample = ss[p]
    ts = _tsim(t, 7)
    paths, idx = sample.simulate_paths(ts, 8, "random", seed=1, return_index=True)
    assert paths.shape == (8, 7) and idx.shape == (8,) and np.all((idx >= 0) & (idx < 200)) and np.all(np.isfinite(paths))
    assert np.array_equal(idx, np.random.RandomState(1).randint(0, 200, size=8)) and len(set(idx.tolist())) > 1
    p2, idx2 = sample.simulate_paths(ts, 8, "random", seed=1, return_index=True)
    assert np.array_equal(p2, paths) and np.array_equal(idx2, idx)
    assert not np.array_equal(sample.simulate_paths(ts, 8, "random", seed=2), paths)
    sig = np.ravel(sample._samples["sigma"])
    mus = np.ravel(sample._samples["mu"])
    if p == 1:
        om = np.exp(np.ravel(sample._samples["log_omega"])[idx])
    for j, i in enumerate(idx):                                          # row j = sample idx[j]'s model at path j
        if p == 1:
            want = lib.simulate_cond_car1(t, y, e, sig[i:i + 1] ** 2, om[j:j + 1], mus[i:i + 1], ts, seed=1, path0=j)
        else:
            want = lib.simulate_cond_carma(t, y, e, sig[i:i + 1] ** 2, sample._samples["ar_roots"][i:i + 1],
                                           sample._samples["ma_coefs"][i:i + 1], mus[i:i + 1], ts, seed=1, path0=j)
        assert np.array_equal(paths[j], want[0]), j
    # one model for every row
    for bestfit in ("map", 17):
        rows, none = sample.simulate_paths(ts, 4, bestfit, seed=3, return_index=True)
        assert none is None and rows.shape == (4, 7) and len({r.tobytes() for r in rows}) == 4
        kf, mu = sample.makeKalmanFilter(bestfit)
        assert np.array_equal(kf.SimulateBatch(ts, 4, seed=3) + mu, rows)
        assert np.array_equal(np.asarray(kf.SimulateBatch(cm.vecD(ts.tolist()), 4, seed=3)) + mu, rows)
    # seed None: numpy's global stream
    np.random.seed(11)
    a = sample.simulate_paths(ts, 3)
    np.random.seed(11)
    assert np.array_equal(sample.simulate_paths(ts, 3), a) and a.shape == (3, 7)
    np.random.seed(12)
    b = kf.SimulateBatch(ts, 2)
    np.random.seed(12)
    assert np.array_equal(kf.SimulateBatch(ts, 2), b) and b.shape == (2, 7)
    # the reference's loop body
    one = sample.simulate(ts, bestfit="random")
    assert one.shape == (7,) and np.all(np.isfinite(one))
    # the ensemble's spread is the conditional one: the map rows against predict (5 sigma of the sampling error of 256 paths)
    rows = sample.simulate_paths(ts, 256, "map", seed=4)
    pm, pv = sample.predict(ts, bestfit="map")
    assert np.all(np.abs(rows.mean(axis=0) - pm) <= 5.0 * np.sqrt(pv / 256))
