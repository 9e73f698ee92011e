"""GPU tests of the sampler over a SET of multi-band objects (k_logdens_carma_mband_chains_ms behind carma_bandset_pt_*,
BandsSetContext.pt_*, CarmaBandsSet.run_mcmc).

The yardstick is the single object's sampler (carma_bands_pt_*, BandsContext.pt_*), which tests/test_gpu_mband_pt.py holds to the
reference ladder and to lag recovery.  A wave of the set's K1 works on one object with the body of the single object's K1, the
bookkeeping kernels are the same launches on an ensemble of the same shape and every key is positional (chain = ladder T +
temperature), so run j of M runs of R replicas is held to BIT equality with ladders j R ... j R + R - 1 of a BandsContext on its
object alone with M R replicas: np.array_equal everywhere, no tolerance.

The objects are the four of tests/test_gpu_mbandset.py (N = 6, 20, 40, 600 in three bands; a band of one datum; equal shifted
times).  With three bands the orders (2,1), (5,3), (7,6) have dx = 12, 17, 22: the fused templated bookkeeping and the wide one
twice."""
import functools

import numpy as np
import pytest

import mband_pt_build as pb
import mband_ref as R
from helpers import prior_like_theta
from test_gpu_mbandset import lag_boxes, make_set, objects, single

pytestmark = pytest.mark.gpu

SEED = 20241021
ORDERS = [(1, 0), (2, 1), (5, 3), (7, 6)]
K = 3
RUNS = [3, 0, 2, 0, 1]                                        # an object twice, mixed lengths


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
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def _set(cpa, p, q):
    if ("set", p, q) not in _CTX:
        _CTX[("set", p, q)] = make_set(cpa, p, q)
    return _CTX[("set", p, q)]


def _single(cpa, s, p, q):
    if (s, p, q) not in _CTX:
        _CTX[(s, p, q)] = single(cpa, s, p, q)
    return _CTX[(s, p, q)]


def _temps(T):
    return np.exp(np.log(100.0) * np.arange(T) / max(T - 1, 1))


@functools.lru_cache(None)
def _bands(s):
    return pb.prepared(objects()[0][s])


def _wide_box(cpa, s, p, q):
    """The default box of object s widened to hold its own band terms (as test_gpu_mband_pt._problem widens it)."""
    lo, hi = _single(cpa, s, p, q).pt_default_box()
    val = np.array([(np.log(a), mu) for _, a, mu in objects()[1][s]])
    return np.minimum(lo, val - 1.0), np.maximum(hi, val + 1.0)


def _run_boxes(cpa, runs, p, q):
    """(lo, hi) [M, K - 1, 2]: every run's box; a LATER run on an object seen before gets a narrower box of its own (the top of
    mu of band 2 comes down to the object's value + 0.05)."""
    lo, hi = (np.array(v) for v in zip(*[_wide_box(cpa, s, p, q) for s in runs]))
    for j, s in enumerate(runs):
        if s in runs[:j]:
            hi[j, 1, 1] = objects()[1][s][1][2] + 0.05
    return lo, hi


def _finite_points(cpa, rng, n, s, p, q, box):
    """n extended vectors with a finite log-posterior on object s inside box, built as test_gpu_mband_pt._points builds them."""
    bands, extras = _bands(s), objects()[1][s]
    t0, y0, _ = bands[0]
    ctx = _single(cpa, s, p, q)

    def draw(m):
        x = np.array([R.extend(prior_like_theta(rng, p, q, t0, y0), extras) for _ in range(m)])
        return x + 1e-3 * rng.standard_normal(x.shape)

    x = draw(n)
    for _ in range(200):
        bad = ~(np.isfinite(ctx.logdensity(x, ignore_prior=False)) & pb.in_box(x, ctx.d, K, box))
        if not bad.any():
            return x
        x[bad] = draw(int(bad.sum()))
    raise AssertionError("no finite starting values for object %d at (%d,%d)" % (s, p, q))


# ---- 1. K1 bits and the box ------------------------------------------------------------------------------------------------------
def _k1_vectors(rng, s, n, p, q, box):
    """n vectors of object s as test_gpu_mbandset.problem() builds them: jittered CARMA parts and band terms, some outside the
    prior, a lag outside its box, a NaN band term -- and some band terms outside the run's band box."""
    objs, extras = objects()
    base = R.order_thetas(p, q)
    t0 = objs[s][0][0]
    d = 3 + p + q
    rows = []
    for i in range(n):
        th = base[i % 2].copy()
        if p == 1:
            th[3] = 0.5 * (np.log(1.0 / np.diff(t0).min()) + np.log(1.0 / (t0.max() - t0.min())))
        ex = [list(e) for e in extras[s]]
        if i >= 2:
            th[:3] += [0.1 * rng.uniform(), 0.05 * rng.uniform(), 0.2 * rng.standard_normal()]
            for e in ex:
                e[0] += 0.25 * rng.integers(-3, 4)
                e[1] *= 1.0 + 0.2 * rng.uniform()
                e[2] += 0.3 * rng.standard_normal()
        x = R.extend(th, ex)
        if i >= 2 and i % 9 == 3:
            x[0] = 1e3                                       # ysigma above max_stdev
        if i >= 2 and i % 9 == 5:
            x[d] += 7.0                                      # lag 1 above its box
        if i >= 2 and i % 17 == 8:
            x[d + 4] = np.nan                                # log a of band 2
        if i >= 2 and i % 7 == 4:
            x[d + 1] = box[1][0, 0] + 1e-6                   # log a of band 1 just above the run's box
        if i >= 2 and i % 11 == 6:
            x[d + 5] = box[0][1, 1] - 1e-6                   # mu of band 2 just below it
        rows.append(x)
    return np.array(rows)


@pytest.mark.parametrize("T,Rr", [(3, 3), (10, 1), (64, 1), (10, 13)])
@pytest.mark.parametrize("p,q", ORDERS)
def test_k1_has_the_bits_of_the_single_objects_k1_and_each_runs_box(cpa, p, q, T, Rr):
    st = _set(cpa, p, q)
    d, dx, RT, M = st.d, st.dx, T * Rr, len(RUNS)
    assert RT in (9, 10, 64, 130)
    lo, hi = _run_boxes(cpa, RUNS, p, q)
    assert not np.array_equal(hi[1], hi[3])                  # the two runs on object 0 have boxes of their own
    rng = np.random.default_rng(1000 * p + 10 * q + RT)
    th = np.empty((M, RT, dx))
    for j, s in enumerate(RUNS):
        th[j] = _k1_vectors(rng, s, RT, p, q, (lo[j], hi[j]))
    th[3] = th[1]                                            # the same vectors in both runs on object 0 ...
    th[3, 2:, d + 5] = np.where(np.arange(2, RT) % 2 == 0, hi[3, 1, 1] + 0.01, th[3, 2:, d + 5])   # ... some between the two tops
    st.pt_create(RUNS, T, Rr, 5, seed=1, band_box=(lo, hi))
    assert st.pt_kernel_name() == "k_logdens_carma_mband_chains_ms<%d>" % p
    got = st.pt_logdensity(th.reshape(M, Rr, T, dx)).reshape(M, RT)      # (the guard words are the entry point's check)
    assert not np.isnan(got).any()
    nfin = 0
    for j, s in enumerate(RUNS):
        ctx = _single(cpa, s, p, q)
        ctx.pt_create(T, Rr, 5, seed=1, band_box=(lo[j], hi[j]))
        want = ctx.pt_logdensity(th[j].reshape(Rr, T, dx)).ravel()
        assert np.array_equal(got[j], want), (j, s, np.flatnonzero(got[j] != want)[:4])
        inside = pb.in_box(th[j], d, K, (lo[j], hi[j]))
        plain = np.where(inside, ctx.logdensity(np.where(np.isnan(th[j]), 0.0, th[j]), ignore_prior=False), -np.inf)
        plain[np.isnan(th[j]).any(axis=1)] = -np.inf
        assert np.array_equal(got[j], plain), (j, s)
        assert RT < 9 or (np.isneginf(got[j]).any() and not inside.all())
        nfin += int(np.isfinite(got[j]).sum())
    assert nfin > 0
    # run 3 obeys ITS box: the vectors between the two tops are finite in run 1 and -inf in run 3
    between = (th[3][:, d + 5] > hi[3, 1, 1]) & pb.in_box(th[3], d, K, (lo[1], hi[1]))
    assert between.any() and np.all(np.isneginf(got[3][between]))
    same = np.all(th[1] == th[3], axis=1) & (th[3][:, d + 5] <= hi[3, 1, 1])
    assert np.array_equal(got[1][same], got[3][same])
    # no box at all: nothing but the library's log-density of each run's object
    st.pt_create(RUNS, T, Rr, 5, seed=1)
    free = st.pt_logdensity(th.reshape(M, Rr, T, dx)).reshape(M * RT)
    assert np.array_equal(free, st.logdensity(th.reshape(M * RT, dx), np.repeat(RUNS, RT), ignore_prior=False), equal_nan=True)


# ---- 2. a run walks its own object's trajectory -----------------------------------------------------------------------------------
def _counts(ctx):
    a, w = ctx.pt_stats()
    n = ctx.pt_iterations_done()
    return np.rint(a * n).astype(np.int64), np.rint(w * n).astype(np.int64)


def _walk(ctx, parts, ns, thin):
    for n in parts:
        ctx.pt_iterate(n, True)
    th1, lp1 = ctx.pt_get_chains()
    f1 = ctx.pt_get_factor()
    sm, sl = ctx.pt_sample(ns, thin)
    th2, lp2 = ctx.pt_get_chains()
    acc, swp = _counts(ctx)
    return dict(th1=th1, lp1=lp1, f1=f1, sm=sm, sl=sl, th2=th2, lp2=lp2, f2=ctx.pt_get_factor(), acc=acc, swp=swp)


KEYS = ("th1", "lp1", "f1", "sm", "sl", "th2", "lp2", "f2", "acc", "swp")


def _set_walk(cpa, p, q, runs, T, Rr, starts, boxes, parts=(40,), ns=20, thin=2, adapt=40):
    st = _set(cpa, p, q)
    st.pt_create(runs, T, Rr, adapt, seed=SEED, temperatures=_temps(T), band_box=boxes)
    st.pt_set_chains(np.array(starts).reshape(len(runs), Rr, T, st.dx))
    return _walk(st, parts, ns, thin)


@pytest.mark.parametrize("T", [3, 10])
@pytest.mark.parametrize("p,q", [(2, 1), (5, 3), (7, 6)])
def test_a_run_walks_the_trajectory_of_its_object_alone(cpa, p, q, T):
    runs, Rr = [3, 0, 2], 2
    M, RT = len(runs), Rr * T
    st = _set(cpa, p, q)
    dx = st.dx
    assert dx == {2: 12, 5: 17, 7: 22}[p] and pb.ram_kernels_plan(dx) == (pb.RAM_FUSED if p == 2 else pb.RAM_WIDE)
    lo, hi = _run_boxes(cpa, runs, p, q)
    rng = np.random.default_rng(31 * dx + T)
    # finite starts for a WHOLE ensemble of M R ladders on every run's object: run j of the set takes block j of its own
    full = [_finite_points(cpa, rng, M * RT, s, p, q, (lo[j], hi[j])) for j, s in enumerate(runs)]
    g = _set_walk(cpa, p, q, runs, T, Rr, [full[j][j * RT:(j + 1) * RT] for j in range(M)], (lo, hi))
    assert np.all(np.isfinite(g["lp1"])) and np.all(np.isfinite(g["sl"]))
    assert st.pt_iterations_done() == 40 + 40
    assert g["acc"].sum() > 0 and g["swp"].sum() > 0
    assert g["sm"].shape == (M, Rr, 20, dx) and g["acc"].shape == (M, Rr, T)
    for j, s in enumerate(runs):
        ctx = _single(cpa, s, p, q)
        ctx.pt_create(T, M * Rr, 40, seed=SEED, temperatures=_temps(T), band_box=(lo[j], hi[j]))
        ctx.pt_set_chains(full[j].reshape(M * Rr, T, dx))
        w = _walk(ctx, (40,), 20, 2)
        for k in KEYS:
            assert np.array_equal(g[k][j], w[k][j * Rr:(j + 1) * Rr]), (j, s, k)
        assert not np.array_equal(w["th1"][j * Rr:(j + 1) * Rr].reshape(RT, dx), full[j][j * RT:(j + 1) * RT])
        assert not np.array_equal(w["f1"][j * Rr], np.broadcast_to(pb.initial_factor(_bands(s), ctx.d), w["f1"][j * Rr].shape))


# ---- 3. a run does not depend on its neighbours ------------------------------------------------------------------------------------
def test_a_run_has_the_same_bits_whatever_its_neighbours_and_chunks_are(cpa):
    p, q, T, Rr = 5, 3, 10, 2
    RT = Rr * T
    a_runs, b_runs = [3, 0, 2], [1, 0, 3]
    rng = np.random.default_rng(77)
    box = {s: _wide_box(cpa, s, p, q) for s in range(4)}
    pts = {s: _finite_points(cpa, rng, RT, s, p, q, box[s]) for s in range(4)}

    def run(runs, parts):
        lo, hi = (np.array(v) for v in zip(*[box[s] for s in runs]))
        return _set_walk(cpa, p, q, runs, T, Rr, [pts[s] for s in runs], (lo, hi), parts=parts, ns=6, thin=2, adapt=45)

    a, b, c = run(a_runs, (60,)), run(b_runs, (60,)), run(a_runs, (25, 35))
    for k in KEYS:
        assert np.array_equal(a[k][1], b[k][1]), k            # object 0 at position 1 of both lists
        assert np.array_equal(a[k], c[k]), k                  # one iterate(60) = iterate(25) + iterate(35)
    assert not np.array_equal(a["th1"][0], b["th1"][0])


# ---- 4. starts ----------------------------------------------------------------------------------------------------------------------
def test_starts_are_the_single_contexts_and_an_init_row_is_honoured(cpa):
    p, q, T, Rr = 2, 1, 10, 2
    runs = [2, 3]
    M, RT = len(runs), Rr * T
    st = _set(cpa, p, q)
    dx, d = st.dx, st.d
    lo, hi = _run_boxes(cpa, runs, p, q)
    st.pt_create(runs, T, Rr, 10, seed=SEED, band_box=(lo, hi))
    st.pt_start()
    th, lp = st.pt_get_chains()
    assert th.shape == (M, Rr, T, dx) and np.all(np.isfinite(lp))
    for j, s in enumerate(runs):
        assert pb.in_box(th[j].reshape(RT, dx), d, K, (lo[j], hi[j])).all()
        ctx = _single(cpa, s, p, q)
        assert np.array_equal(lp[j].ravel(), ctx.logdensity(th[j].reshape(RT, dx), ignore_prior=False))
        ctx.pt_create(T, M * Rr, 10, seed=SEED, band_box=(lo[j], hi[j]))
        ctx.pt_start()
        th1, lp1 = ctx.pt_get_chains()
        assert np.array_equal(th[j], th1[j * Rr:(j + 1) * Rr]) and np.array_equal(lp[j], lp1[j * Rr:(j + 1) * Rr])
    st.pt_iterate(3, True)                                   # the chains are usable
    # an init row with a finite log-posterior becomes every chain of ITS run; the other run draws as before
    rng = np.random.default_rng(5)
    init = np.array([_finite_points(cpa, rng, 1, s, p, q, (lo[j], hi[j]))[0] for j, s in enumerate(runs)])
    init[1, 0] = 1e3                                         # ysigma above max_stdev: -inf on object 3
    st.pt_create(runs, T, Rr, 10, seed=SEED, band_box=(lo, hi))
    st.pt_start(init)
    th2, lp2 = st.pt_get_chains()
    assert np.array_equal(th2[0], np.broadcast_to(init[0], (Rr, T, dx)))
    assert np.all(lp2[0] == _single(cpa, 2, p, q).logdensity(init[0], ignore_prior=False))
    assert np.array_equal(th2[1], th[1]) and np.array_equal(lp2[1], lp[1])
    with pytest.raises(ValueError, match="init"):
        st.pt_start(init[:1])
    # a run that finds no finite start is named: the box of run 1 holds no mu a start is drawn at
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[1, :, 1], hi2[1, :, 1] = 1e6, 2e6
    st.pt_create(runs, T, Rr, 10, seed=SEED, band_box=(lo2, hi2))
    with pytest.raises(ValueError, match=r"carma_bandset_pt_start.*no finite starting value.*run 1 \(object 3\)"):
        st.pt_start()
    with pytest.raises(ValueError, match="no starting values"):
        st.pt_iterate(1, True)


# ---- 5. CarmaBandsSet.run_mcmc ------------------------------------------------------------------------------------------------------
def test_bands_set_run_mcmc(cpa):
    p, q, ns, Rr = 2, 1, 60, 2
    bset = cpa.CarmaBandsSet(objects()[0], p=p, q=q, lag_bounds=lag_boxes())
    which = [3, 1]
    out = bset.run_mcmc(ns, nreplicas=Rr, which=which, seed=11)
    dx = bset.dx
    assert isinstance(out, list) and len(out) == 2
    ctx = bset.context()
    boxes = [ctx.pt_default_box(s) for s in which]           # (object 3 is the longer one: the device order is the caller's)
    lo, hi = (np.array(v) for v in zip(*boxes))
    samples, logposts = ctx.pt_run(which, 10, Rr, ns, ns // 2, 1, seed=11, band_box=(lo, hi))
    for i, s in enumerate(which):
        smp, model = out[i], bset.models[s]
        assert isinstance(smp, cpa.CarmaBandsSample) and model.mcmc_sample is smp and smp.model is model
        got = smp._all[0]
        assert got.shape == (Rr, ns, dx)
        assert np.array_equal(got, samples[i]) and np.array_equal(smp._all[1], logposts[i])
        for name in ("lag", "scale", "offset"):
            assert smp.get_samples(name).shape == (Rr * ns, K - 1)
        assert np.array_equal(smp.get_samples("lag"), got.reshape(-1, dx)[:, bset.d + 3 * np.arange(K - 1)])
        assert np.array_equal(smp.get_samples("loglik")[:, 0], model.loglik(got.reshape(-1, dx)))
        assert np.array_equal(smp.get_samples("logpost")[:, 0], logposts[i].ravel())
        assert np.all(np.isfinite(smp.get_samples("sigma"))) and np.all(np.isfinite(smp.get_samples("loglik")))
        lb = lag_boxes()[s]
        med, lo_, hi_ = smp.lag_summary()
        assert med.shape == (K - 1,) and np.all((lo_ <= med) & (med <= hi_)) and np.all((med >= lb[:, 0]) & (med <= lb[:, 1]))
        t = np.linspace(model.bands[0][0][0], model.bands[0][0][-1], 7)
        bm, bv = smp.smooth_band(t, band=1, nsamples=16)
        assert bm.shape == bv.shape == (7,) and np.all(np.isfinite(bm)) and np.all(bv > 0)
    assert bset.models[0].mcmc_sample is None and bset.models[2].mcmc_sample is None
    # which=None: every object, in the caller's order
    allout = bset.run_mcmc(8, nburnin=4, which=None, seed=3)
    assert len(allout) == 4 and all(bset.models[s].mcmc_sample is allout[s] for s in range(4))
    assert [o._all[0].shape for o in allout] == [(1, 8, dx)] * 4
    for m in bset.models:
        if m._ctx is not None:
            m._ctx.close()
    ctx.close()


# ---- 6. calls out of order -------------------------------------------------------------------------------------------------------------
def test_calls_out_of_order_are_einval_with_a_message(cpa):
    lib, last_error = cpa._lib.lib, cpa._lib.last_error
    st = make_set(cpa, 2, 1)
    h, dx = st.handle, st.dx
    buf = np.zeros(4 * 2 * 3 * dx * dx)
    ptr = cpa._lib.ptr
    before = [("set_chains", (ptr(buf), None)), ("get_chains", (ptr(buf), ptr(buf))), ("start", (None,)), ("get_factor", (ptr(buf),)),
              ("set_factor", (ptr(buf),)), ("iterate", (1, 1)), ("sample", (1, 1, ptr(buf), ptr(buf))), ("stats", (ptr(buf), ptr(buf), 0)),
              ("logdensity", (ptr(buf), ptr(buf)))]
    for name, args in before:
        assert getattr(lib, "carma_bandset_pt_" + name)(h, *args) == cpa._lib.CARMA_EINVAL, name
        assert "carma_bandset_pt_%s: call carma_bandset_pt_create first" % name in last_error()
    assert lib.carma_bandset_pt_iterations_done(h) == cpa._lib.CARMA_EINVAL
    with pytest.raises(ValueError, match="pt_create first"):
        st.pt_get_chains()
    # created, not started: iterate and sample are refused, the rest works; the handle stays usable
    st.pt_create([1, 0], 3, 2, 5, seed=1)
    for name, args in (("iterate", (1, 1)), ("sample", (1, 1, ptr(buf), ptr(buf)))):
        assert getattr(lib, "carma_bandset_pt_" + name)(h, *args) == cpa._lib.CARMA_EINVAL, name
        assert "chains have no starting values" in last_error()
    assert st.pt_iterations_done() == 0 and st.pt_get_factor().shape == (2, 2, 3, dx, dx)
    with pytest.raises(ValueError, match=r"run 1 \(object 4\)"):
        st.pt_create([1, 4], 3, 2, 5)
    with pytest.raises(ValueError, match=r"run 0 \(object 1\).*temperatures"):
        st.pt_create([1, 0], 65, 2, 5)
    st.pt_create([1, 0], 3, 2, 5, seed=1)
    st.pt_start()
    st.pt_iterate(2, True)
    assert st.pt_iterations_done() == 2
    assert np.isfinite(st.logdensity(st.pt_get_chains()[0].reshape(-1, dx), np.repeat([1, 0], 6))).all()
    st.close()
