"""GPU tests of the sampler over many series (carma_mpt_*, MultiContext.pt_*, CarmaModelSet.run_mcmc, get_mle(starts="set")).

A RUN is one sampler (R replicas x T temperatures) on one series; the M runs of a call are the ladders j R ... j R + R - 1 of one
ensemble of M R ladders, with the random streams keyed by a chain's place in that ensemble.  So run j must walk, bit for bit,
the block replica0 = j R of a single-series lane-sampler ensemble on its series -- which is what most tests here lean on."""
import ctypes as C
import re

import numpy as np
import pytest

import oracle as orc
from helpers import assert_parity, irregular_series, loglik_truth, theta_batch

pytestmark = pytest.mark.gpu

RTOL = 1e-10
SEED = 20240611
# the series of run j: any order is allowed, an ensemble's neighbours differ in length (n = 270, 33, 300 regular, 20, 700, ...)
RUNS = [4, 1, 7, 0, 5, 2, 8, 6, 3]
CHECKED = (0, 2, 4)     # runs compared with single-series samplers: n = 270, the regular-cadence n = 300, n = 700 (all >= 64: CAR(1))
# (p, q, T, R): T = 3 -- 21 ladders per wave, one lane idle; T = 10 -- the default, 4 idle; T = 64; T = 1 for p = 1.  R leaves the last
# wave partly filled where T allows it, and every wave of T < 64 holds ladders of runs with different n.  d = 16 at (7, 6): beyond
# the proposal fused into the finish kernel (d <= 12).
LADDERS = [(1, 0, 1, 7), (1, 0, 3, 5), (2, 1, 3, 5), (5, 3, 10, 2), (5, 3, 64, 1), (7, 6, 10, 2)]


@pytest.fixture(scope="module")
def cpa():
    import carma_pack_amd
    assert carma_pack_amd._lib.lib.carma_device_count() >= 1, "no MI355X visible"
    return carma_pack_amd


def _series_set():
    out = [irregular_series(n, seed=600 + i) for i, n in enumerate([20, 33, 64, 100, 270, 700])]
    for i, n in enumerate([50, 300]):                         # regular cadence with a gap (REPDT)
        rng = np.random.default_rng(650 + i)
        t = 0.5 * np.arange(n, dtype=float)
        t[n // 2:] += 7.25
        out.append((t, 10.0 + np.sin(t / 5.0) + 0.3 * rng.standard_normal(n), np.full(n, 0.3)))
    t, y, e = irregular_series(120, seed=660)                  # unsorted, with duplicate times
    dup = np.arange(0, 120, 5)
    t, y, e = np.concatenate([t, t[dup]]), np.concatenate([y, y[dup] + 0.1]), np.concatenate([e, e[dup]])
    perm = np.random.default_rng(3).permutation(t.size)
    out.append((t[perm], y[perm], e[perm]))
    return out


@pytest.fixture(scope="module")
def sset():
    return _series_set()


_MC = {}


def _mctx(cpa, sset, p, q):
    """One MultiContext per order for the whole module (its sampler is re-created by every pt_create)."""
    if (p, q) not in _MC:
        _MC[(p, q)] = cpa.MultiContext(sset, p, q)
    return _MC[(p, q)]


def _started(mc, runs, T, R, adapt, seed=SEED, init=None):
    """pt_create + pt_start; a series without a finite start at this order may be dropped, once, by name."""
    runs = list(runs)
    dropped = []
    while True:
        mc.pt_create(runs, T, R, adapt, seed=seed)
        try:
            mc.pt_start(init)
            return runs, dropped
        except ValueError as exc:
            m = re.search(r"\(series (\d+)\)", str(exc))
            assert m and not dropped, "more than one series without a finite start: %s" % exc
            dropped.append(int(m.group(1)))
            print("p=%d q=%d: series %d dropped: no finite start" % (mc.p, mc.q, dropped[0]))
            runs = [s for s in runs if s != dropped[0]]
            assert init is None


def _big(cpa, mc, s, T, R, j, adapt, seed=SEED):
    """The single-series lane-sampler ensemble whose block replica0 = j R run j must equal: >= 70 000 chains."""
    t, y, e = mc.data(s)
    ctx = cpa.Context(t, y, e, mc.p, mc.q, max_stdev=mc.prior(s)[0])
    assert ctx.prior() == mc.prior(s) and ctx.n == mc.n[s]
    Rb = max(-(-70000 // T), (j + 1) * R)
    Rb = -(-Rb // R) * R                                      # whole tiles of the run
    name = ctx.kernel_name(Rb * T)
    assert name.startswith("k_logdens_car1" if mc.p == 1 else "k_logdens_carma_lane<%d" % mc.p) and "scan" not in name, name
    ctx.pt_create(T, Rb, adapt, seed=seed)
    assert cpa._lib.lib.carma_pt_kernel_in_use(ctx.handle) == 2
    return ctx, Rb


# ---- 0. the log-density kernel on its own ---------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q", [(1, 0), (2, 1), (3, 0), (4, 3), (5, 3), (6, 0), (7, 6)])
def test_chain_kernel_has_the_bits_of_the_wave_per_series_kernel(cpa, sset, p, q):
    """A chain's value is what k_logdens_carma_lane_ms (and so the single-series lane kernel: test_gpu_mseries.py) gives, bit
    for bit, on irregular and regular-cadence series, -inf included; lanes past the last chain write nothing (the entry point
    checks the words behind its results)."""
    mc = _mctx(cpa, sset, p, q)
    rng = np.random.default_rng(17 * p + q)
    for T, R in ((10, 2), (3, 5), (64, 1)):
        mc.pt_create(RUNS, T, R, 5, seed=1)
        assert mc.pt_kernel_name() == ("k_logdens_car1_chains_ms" if p == 1 else "k_logdens_carma_chains_ms<%d>" % p)
        assert T == 64 or (len(RUNS) * R * T) % 64 != 0        # a partly filled last wave
        th = np.stack([theta_batch(rng, R * T, p, q, sset[s][0], sset[s][1]) for s in RUNS]).reshape(len(RUNS), R, T, mc.d)
        th[::2, 0, 0, 1] = 5.0                                # error scale outside its bounds: -inf
        got = mc.pt_logdensity(th)
        want = mc.logdensity(th.reshape(-1, mc.d), np.repeat(RUNS, R * T)).reshape(got.shape)
        assert np.isfinite(got).any() and np.isneginf(got).any()
        assert np.array_equal(got, want), (T, R, np.argwhere(got != want)[:4])


# ---- 1. the single-series lane sampler's trajectory ----------------------------------------------------------------------
@pytest.mark.parametrize("p,q,T,R", LADDERS)
def test_run_walks_the_single_series_lane_samplers_trajectory(cpa, sset, p, q, T, R):
    mc = _mctx(cpa, sset, p, q)
    adapt, niter = 25, 40                                     # adapting and frozen iterations
    runs, dropped = _started(mc, RUNS, T, R, adapt)
    assert not dropped or dropped[0] not in [RUNS[j] for j in CHECKED]
    th0, lp0 = mc.pt_get_chains()
    f0 = mc.pt_get_factor()
    bigs = []
    for j in [runs.index(RUNS[j]) for j in CHECKED]:
        ctx, Rb = _big(cpa, mc, runs[j], T, R, j, adapt)
        reps = Rb // R
        ctx.pt_set_chains(np.tile(th0[j], (reps, 1, 1)), np.tile(lp0[j], (reps, 1)))
        assert np.array_equal(ctx.pt_get_factor()[j * R:(j + 1) * R], f0[j]), "initial factor of run %d" % j
        bigs.append((j, ctx))
    mc.pt_iterate(niter, True)
    th1, lp1 = mc.pt_get_chains()
    f1 = mc.pt_get_factor()
    a1, w1 = mc.pt_stats()
    sm, sl = mc.pt_sample(5, 3)
    th2, lp2 = mc.pt_get_chains()
    assert mc.pt_iterations_done() == niter + 15
    for j, ctx in bigs:
        blk = slice(j * R, (j + 1) * R)
        what = "p=%d q=%d T=%d run %d (series %d, n=%d)" % (p, q, T, j, runs[j], mc.n[runs[j]])
        ctx.pt_iterate(niter, True)
        bt, bl = ctx.pt_get_chains()
        assert np.array_equal(th1[j], bt[blk]) and np.array_equal(lp1[j], bl[blk]), what
        assert np.array_equal(f1[j], ctx.pt_get_factor()[blk]), what + ": factors"
        ba, bw = ctx.pt_stats()
        assert np.array_equal(a1[j], ba[blk]) and np.array_equal(w1[j], bw[blk]), what + ": accept / swap counts"
        bs, bsl = ctx.pt_sample(5, 3)
        assert np.array_equal(sm[j], bs[blk]) and np.array_equal(sl[j], bsl[blk]), what + ": saved samples"
        bt, bl = ctx.pt_get_chains()
        assert np.array_equal(th2[j], bt[blk]) and np.array_equal(lp2[j], bl[blk]), what + ": after sampling"
        assert a1[j].max() > 0 and np.isfinite(lp2[j]).all()
        ctx.close()


# ---- 2. a run's samples belong to its own series -------------------------------------------------------------------------
def _check_against_oracle(mc, sset, s, samples, logposts, p, q, what):
    t, y, e = sset[s]
    tt, yy, ee = mc.data(s)
    want = orc.OracleModel(t, y, e, p, q, max_stdev=mc.prior(s)[0]).logdensity_batch(samples)
    assert np.isfinite(logposts).all(), what
    arb = (lambda i: loglik_truth(tt, yy, ee, samples[i], p, q)[0]) if p > 1 else None
    assert_parity(logposts, want, RTOL, what, arbiter=arb)


@pytest.mark.parametrize("p,q,T,R", [(1, 0, 1, 7), (2, 1, 3, 5), (5, 3, 10, 2), (7, 6, 10, 2)])
def test_saved_samples_are_on_the_runs_own_series(cpa, sset, p, q, T, R):
    mc = _mctx(cpa, sset, p, q)
    runs, _ = _started(mc, RUNS, T, R, 20)
    mc.pt_iterate(20, True)
    sm, sl = mc.pt_sample(30, 1)
    assert sm.shape == (len(runs), R, 30, mc.d)
    for j, s in enumerate(runs):
        _check_against_oracle(mc, sset, s, sm[j].reshape(-1, mc.d), sl[j].ravel(), p, q, "p=%d q=%d run %d series %d" % (p, q, j, s))


# ---- 3. a run does not depend on its neighbours --------------------------------------------------------------------------
@pytest.mark.parametrize("p,q,T,R", [(2, 1, 3, 5), (5, 3, 10, 2)])
def test_run_does_not_depend_on_its_neighbours(cpa, sset, p, q, T, R):
    mc = _mctx(cpa, sset, p, q)

    def run(runs):
        mc.pt_create(runs, T, R, 25, seed=SEED)
        mc.pt_start()
        mc.pt_iterate(30, True)
        sm, sl = mc.pt_sample(4, 2)
        return mc.pt_get_chains() + (mc.pt_get_factor(), sm, sl)

    a = run([5, 3, 0])                                       # n = 700, 100, 20
    b = run([0, 3, 5])                                       # n = 20, 100, 700
    for x, y in zip(a, b):
        assert np.array_equal(x[1], y[1])
        assert not np.array_equal(x[0], y[2])
    twice = run([3, 3])
    for x in twice:
        assert np.isfinite(x).all() and not np.array_equal(x[0], x[1])


# ---- 3b. a second, smaller sampling call --------------------------------------------------------------------------------
def test_a_second_smaller_sample_call_continues_the_first(cpa):
    """pt_sample(8) and then pt_sample(3) on one sampler: the second call writes into the buffer the first one sized, with a stride
    of its own.  Together they are the 11 samples one call gives from the same seed and chains, bit for bit."""
    mc = cpa.MultiContext([irregular_series(30, seed=671), irregular_series(64, seed=672)], 2, 1)
    runs, T, R = [0, 1], 3, 2
    mc.pt_create(runs, T, R, 10 ** 6, seed=SEED)
    mc.pt_start()
    th0, lp0 = mc.pt_get_chains()
    s8, l8 = mc.pt_sample(8, 2)
    s3, l3 = mc.pt_sample(3, 2)
    th1, lp1 = mc.pt_get_chains()
    mc.pt_create(runs, T, R, 10 ** 6, seed=SEED)
    mc.pt_set_chains(th0, lp0)
    s11, l11 = mc.pt_sample(11, 2)
    assert s8.shape == (2, R, 8, mc.d) and s3.shape == (2, R, 3, mc.d) and l3.shape == (2, R, 3)
    assert np.array_equal(s8, s11[:, :, :8]) and np.array_equal(l8, l11[:, :, :8])
    assert np.array_equal(s3, s11[:, :, 8:]) and np.array_equal(l3, l11[:, :, 8:])
    assert np.isfinite(l11).all() and not np.array_equal(s11[:, :, 0], s11[:, :, 10])
    th2, lp2 = mc.pt_get_chains()
    assert np.array_equal(th1, th2) and np.array_equal(lp1, lp2)


# ---- 4. chunking is invisible --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q,T,R", [(2, 1, 3, 5), (5, 3, 10, 2), (7, 6, 10, 2)])
def test_iterations_do_not_depend_on_how_they_are_split(cpa, sset, p, q, T, R):
    mc = _mctx(cpa, sset, p, q)
    runs, _ = _started(mc, RUNS, T, R, 25)
    th0, lp0 = mc.pt_get_chains()
    mc.pt_iterate(40, True)
    one = mc.pt_get_chains() + (mc.pt_get_factor(),) + mc.pt_stats()
    mc.pt_create(runs, T, R, 25, seed=SEED)
    mc.pt_set_chains(th0, lp0)
    mc.pt_iterate(13, True)
    mc.pt_iterate(27, True)
    two = mc.pt_get_chains() + (mc.pt_get_factor(),) + mc.pt_stats()
    for x, y in zip(one, two):
        assert np.array_equal(x, y)


# ---- 5. starting values --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q,T,R", [(1, 0, 1, 7), (2, 1, 3, 5), (5, 3, 10, 2), (7, 6, 10, 2)])
def test_starts_are_the_sharded_single_series_starts(cpa, sset, p, q, T, R):
    mc = _mctx(cpa, sset, p, q)
    runs, _ = _started(mc, RUNS, T, R, 25)
    th0, lp0 = mc.pt_get_chains()
    assert np.isfinite(lp0).all()
    for j in (0, 1, len(runs) - 1):
        s = runs[j]
        t, y, e = mc.data(s)
        ctx = cpa.Context(t, y, e, p, q, max_stdev=mc.prior(s)[0])
        ctx.pt_create(T, R, 25, seed=SEED)
        ctx.pt_shard(T, 0, j * R)
        ctx.pt_start()
        bt, bl = ctx.pt_get_chains()
        assert np.array_equal(th0[j], bt), "run %d (series %d)" % (j, s)
        assert_parity(lp0[j].ravel(), bl.ravel(), RTOL, "start log-posteriors, run %d" % j)
        ctx.close()
    # init rows: a finite one is every chain of its run; a non-finite one leaves that run -- and only it -- to the draws
    init = th0[:, 0, 0, :].copy()
    init[1, 1] = 5.0                                         # measurement-error scale outside (0.5, 2): log-density -inf
    mc.pt_create(runs, T, R, 25, seed=SEED)
    mc.pt_start(init)
    th1, lp1 = mc.pt_get_chains()
    for j in range(len(runs)):
        if j == 1:
            assert np.array_equal(th1[j], th0[j]) and np.array_equal(lp1[j], lp0[j])
        else:
            assert (th1[j] == init[j]).all() and (lp1[j] == lp0[j, 0, 0]).all()


# ---- 6. the Python interface ---------------------------------------------------------------------------------------------
def test_model_set_run_mcmc(cpa, sset):
    import carmcmc as cm
    series = [sset[1], sset[4], sset[7], sset[0]]             # n = 33, 270, 300 (regular), 20: not in order of length
    mset = cm.CarmaModelSet(series, 5, 3)
    out = mset.run_mcmc(40, nburnin=30, seed=1)
    assert len(out) == 4 and mset.mcmc_samples is out
    mc = mset.context(5, 3)
    for s, smp in enumerate(out):
        assert isinstance(smp, cm.CarmaSample) and mset.models[s].mcmc_sample is smp
        assert smp.get_samples("var").shape[0] == 40 and smp._samples["loglik"].shape[0] == 40
        assert np.isfinite(smp._samples["loglik"]).all()
        assert smp.get_samples("psd_centroid").shape == (40, 5)
        tn = np.linspace(mset.models[s].time[0], mset.models[s].time[-1] + 5.0, 7)
        pm, pv = smp.predict(tn)
        assert np.isfinite(pm).all() and (np.asarray(pv) > 0).all()
        trace = np.array(smp._sampler.getSamples())
        assert trace.shape == (40, 11)
        # the caller's order although the series ran longest first: the trace is a posterior sample of ITS series
        if s in (0, 1):
            _check_against_oracle(mc, series, s, trace, np.array(smp._sampler.GetLogLikes()), 5, 3, "run_mcmc series %d" % s)
            assert np.array_equal(smp._samples["loglik"].ravel(), mc.logdensity(trace, s, ignore_prior=True))
    again = cm.CarmaModelSet(series, 5, 3).run_mcmc(40, nburnin=30, seed=1)
    for a, b in zip(out, again):
        assert np.array_equal(np.array(a._sampler.getSamples()), np.array(b._sampler.getSamples()))
        assert np.array_equal(a._samples["logpost"], b._samples["logpost"])
        assert np.array_equal(a._samples["loglik"], b._samples["loglik"])
    c1 = cm.CarmaModelSet(series, 1, 0).run_mcmc(20, seed=2)
    assert len(c1) == 4 and all(isinstance(x, cm.Car1Sample) for x in c1)
    assert all(np.isfinite(x._samples["loglik"]).all() and x._samples["log_omega"].shape[0] == 20 for x in c1)


def test_model_set_get_mle_with_the_sets_starts(cpa, sset):
    import carmcmc as cm
    series = [sset[1], sset[4], sset[7]]
    for p, q in ((1, 0), (3, 1)):
        mset = cm.CarmaModelSet(series, p, q)
        best = mset.get_mle(p, q, ntrials=8, seed=3, starts="set")
        assert len(best) == 3 and set(mset.timing) == {"starts_s", "optimise_s"} and mset.timing["starts_s"] > 0
        for s, r in enumerate(best):
            for xj, (lo, hi) in zip(r.x, mset.models[s]._mle_bounds(p, q)):
                assert lo is None or lo <= xj <= hi, (s, r.x)
            assert abs(mset.loglik(r.x, s) + r.fun) <= 1e-10 * abs(r.fun)
        # the default is what it was: the per-model draws, optimised together
        starts = np.stack([m._mle_problem(p, q, 8, 3)[1] for m in mset.models])
        dflt, given = mset.get_mle(p, q, ntrials=8, seed=3), mset.get_mle(p, q, starts=starts)
        for a, b in zip(dflt, given):
            assert np.array_equal(a.x, b.x) and a.fun == b.fun


# ---- 7. error paths ------------------------------------------------------------------------------------------------------
def test_error_paths(cpa, sset):
    lib, EINVAL = cpa._lib.lib, -22
    mc = cpa.MultiContext(sset[:3], 2, 1)
    h = mc.handle
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))                      # noqa: E731
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                   # noqa: E731
    x = np.zeros(4096)
    runs = np.array([0, 2, 1], dtype=np.int32)

    def err(rc, word):
        assert rc == EINVAL and word in cpa._lib.last_error(), (rc, cpa._lib.last_error())

    # before create
    err(lib.carma_mpt_start(h, None), "carma_mpt_create first")
    err(lib.carma_mpt_iterate(h, 1, 1), "carma_mpt_create first")
    err(lib.carma_mpt_sample(h, 1, 1, dp(x), dp(x)), "carma_mpt_create first")
    err(lib.carma_mpt_get_chains(h, dp(x), dp(x)), "carma_mpt_create first")
    err(lib.carma_mpt_stats(h, dp(x), dp(x), 0), "carma_mpt_create first")
    assert lib.carma_mpt_iterations_done(h) == EINVAL
    # create
    err(lib.carma_mpt_create(h, ip(runs), 3, 65, 1, None, 5, C.c_uint64(1)), "64")
    err(lib.carma_mpt_create(h, ip(runs), 3, 0, 1, None, 5, C.c_uint64(1)), "64")
    err(lib.carma_mpt_create(h, ip(runs), 0, 3, 1, None, 5, C.c_uint64(1)), "at least one run")
    err(lib.carma_mpt_create(h, ip(np.array([0, 3, 1], dtype=np.int32)), 3, 3, 1, None, 5, C.c_uint64(1)), "run 1: series index 3")
    err(lib.carma_mpt_create(h, ip(np.array([0, -1, 1], dtype=np.int32)), 3, 3, 1, None, 5, C.c_uint64(1)), "series index -1")
    err(lib.carma_mpt_create(h, ip(runs), 3, 64, 1 << 24, None, 5, C.c_uint64(1)), "chains")
    err(lib.carma_mpt_start(h, None), "carma_mpt_create first")          # nothing was created (or launched) by the bad calls
    with pytest.raises(ValueError):
        mc.pt_create([0, 7], 3, 1, 5)
    # before start
    mc.pt_create(runs, 3, 2, 5, seed=4)
    err(lib.carma_mpt_get_factor(h, None), "carma_mpt_get_factor: null chol")
    err(lib.carma_mpt_set_factor(h, None), "carma_mpt_set_factor: null chol")
    err(lib.carma_mpt_iterate(h, 1, 1), "no starting values")
    err(lib.carma_mpt_sample(h, 1, 1, dp(x), dp(x)), "no starting values")
    mc.pt_start()
    err(lib.carma_mpt_iterate(h, -1, 1), "niter")
    err(lib.carma_mpt_sample(h, 0, 1, dp(x), dp(x)), "nsamples")
    err(lib.carma_mpt_sample(h, 1, 0, dp(x), dp(x)), "thin")
    with pytest.raises(ValueError):
        mc.pt_start(np.zeros((2, mc.d)))
    mc.pt_iterate(3)                                         # the context is still usable
    assert mc.pt_iterations_done() == 3 and np.isfinite(mc.pt_get_chains()[1]).all()
