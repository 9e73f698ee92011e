"""GPU tests of the lock-step optimiser's entry points (carma_mle_batched, carma_mle_batched_ms; the loop itself is held to
objectives with known answers on the CPU, tests/test_mle_loop_cpu.py): every returned start against the oracle -- the value, the
box, the descent, the stationarity of the converged ones --, a start's result independent of what else the call holds, a box
and a series of its own per start, and the status of a start without a finite value."""
import numpy as np
import pytest

import oracle as orc
from helpers import assert_parity, loglik_truth, prior_like_theta

pytestmark = pytest.mark.gpu

RTOL_LP = 1e-10                                              # the project's bar on a log-density
ORDERS = [(1, 0), (2, 1), (5, 3)]
MAXITER, GTOL, FD = 300, 1e-5, 1e-6
NSTARTS = 24


@pytest.fixture(scope="module")
def cpa():
    import carma_pack_amd
    assert carma_pack_amd._lib.lib.carma_device_count() >= 1, "no MI355X visible"
    return carma_pack_amd


def _series(n=80, seed=11):
    """Irregular sampling, a random walk plus noise (as test_gpu_sampler_steps.py)."""
    rng = np.random.default_rng(seed)
    t = np.cumsum(rng.uniform(1.0, 3.0, n))
    y = np.cumsum(rng.standard_normal(n)) * 0.3 + 0.2 * rng.standard_normal(n)
    return t, y - y.mean(), np.full(n, 0.2)


def _box(t, y, e, p, q):
    """get_mle's box as (bounds for Context.mle_batched, lo [d], hi [d])."""
    import carmcmc as cm
    bnds = cm.CarmaModel(t, y, e, p=p, q=q)._mle_bounds(p, q)
    lo = np.array([-np.inf if b[0] is None else b[0] for b in bnds])
    hi = np.array([np.inf if b[1] is None else b[1] for b in bnds])
    return bnds, lo, hi


def _starts(p, q, t, y, n, seed):
    rng = np.random.default_rng(seed)
    x0 = np.array([prior_like_theta(rng, p, q, t, y) for _ in range(n)])
    x0[:, 1] = 1.0                                           # get_mle's initial guess for the error scale
    return x0


_problems = {}


def problem(cpa, p, q):
    """One series, 24 prior-like starts (some outside the box: projected first), the oracle on the same series and prior bound,
    and two runs of carma_mle_batched from them: with the default ftol, and with ftol = 0 so that only the gradient rule can
    end a start.  Computed once per order and shared."""
    if (p, q) not in _problems:
        t, y, e = _series()
        bnds, lo, hi = _box(t, y, e, p, q)
        ctx = cpa.Context(t, y, e, p, q)
        om = orc.OracleModel(t, y, e, p, q, max_stdev=ctx.prior()[0])
        x0 = _starts(p, q, t, y, NSTARTS, 100 * p + q)
        ip = p > 1                                           # get_mle's objective: SetMLE(true) for p > 1
        runs = dict(default=ctx.mle_batched(x0, bnds, maxiter=MAXITER, gtol=GTOL, fd_step=FD, ignore_prior=ip),
                    ftol0=ctx.mle_batched(x0, bnds, maxiter=MAXITER, ftol=0.0, gtol=GTOL, fd_step=FD, ignore_prior=ip))
        with np.errstate(all="ignore"):
            f0 = -om.logdensity_batch(np.clip(x0, lo, hi), ignore_prior=ip)
        for a in (x0, lo, hi, f0) + runs["default"] + runs["ftol0"]:
            a.setflags(write=False)
        _problems[(p, q)] = dict(t=t, y=y, e=e, lo=lo, hi=hi, om=om, x0=x0, ip=ip, f0=f0, runs=runs)
    return _problems[(p, q)]


def _oracle_f(om, pts, ip):
    with np.errstate(all="ignore"):
        return -om.logdensity_batch(np.ascontiguousarray(pts), ignore_prior=ip)


@pytest.mark.parametrize("which", ["default", "ftol0"])
@pytest.mark.parametrize("p,q", ORDERS)
def test_every_start_returns_the_oracles_value_inside_the_box_and_downhill(cpa, p, q, which):
    P = problem(cpa, p, q)
    x, fun, nit, nfev, status = P["runs"][which]
    lo, hi, ip = P["lo"], P["hi"], P["ip"]
    print("p=%d q=%d %s: status counts %s, nit %d ... %d" % (p, q, which, np.bincount(status, minlength=5).tolist(), nit.min(), nit.max()))
    # a start without a finite value at its projected x0 -- by the oracle -- is status 4 and nothing else is
    dead = ~np.isfinite(P["f0"])
    assert np.array_equal(status == 4, dead), (status, dead)
    assert np.all(fun[dead] == 1e300) and np.all(nit[dead] == 0) and np.array_equal(x[dead], np.clip(P["x0"], lo, hi)[dead])
    live = ~dead
    assert live.sum() >= NSTARTS - 4
    assert np.all(fun[live] < 1e299) and np.all(nit[live] > 0) and np.all(nfev[live] > nit[live])
    # EVERY start, not only the best: the value is the oracle's at the returned x
    want = -_oracle_f(P["om"], x[live], ip)
    idx = np.flatnonzero(live)
    arb = (lambda i: loglik_truth(P["t"], P["y"], P["e"], x[idx[i]], p, q)[0]) if p > 1 else None
    worst = assert_parity(-fun[live], want, RTOL_LP, "mle p=%d q=%d %s" % (p, q, which), arbiter=arb)
    print("p=%d q=%d %s: fun against the oracle, worst %.2e" % (p, q, which, worst))
    assert np.all(x >= lo) and np.all(x <= hi)
    # downhill from the projected start (the oracle's value there; the device's may differ from it by the bar)
    f0 = P["f0"][live]
    assert np.all(fun[live] <= f0 + 2.0 * RTOL_LP * np.maximum(1.0, np.abs(f0))), (fun[live] - f0).max()


@pytest.mark.parametrize("p,q", ORDERS)
def test_converged_starts_are_stationary_for_the_oracle(cpa, p, q):
    """For a start that ended on the gradient rule, the ORACLE's central-difference projected gradient at x -- same fd_step,
    same one-sided rule at a bound, same freezing rule -- is within gtol + 2 RTOL_LP max(1, |f|) / (up - dn) per component:
    the second term is what the log-density bar allows two implementations to differ by in a difference quotient (each of
    the two values by RTOL_LP |f|).  The run is the one with ftol = 0: with the default ftol the relative-decrease rule ends
    most starts of this series first (the prototype on the oracle: 13 of 24 on the gradient rule at (1,0), none at (2,1);
    with ftol = 0 all 24 of both)."""
    P = problem(cpa, p, q)
    x, fun, nit, nfev, status = P["runs"]["ftol0"]
    lo, hi, d = P["lo"], P["hi"], x.shape[1]
    conv = np.flatnonzero(status == 0)
    print("p=%d q=%d: %d of %d starts ended on the gradient rule" % (p, q, conv.size, status.size))
    if (p, q) in ((1, 0), (2, 1)):
        assert conv.size >= status.size // 2
    worst = 0.0
    for b in conv:
        h = FD * np.maximum(1.0, np.abs(x[b]))
        up, dn = np.minimum(x[b] + h, hi), np.maximum(x[b] - h, lo)
        pts = np.tile(x[b], (2 * d + 1, 1))
        pts[1 + np.arange(d), np.arange(d)] = up
        pts[1 + d + np.arange(d), np.arange(d)] = dn
        f = _oracle_f(P["om"], pts, P["ip"])
        fu, fd_ = f[1:d + 1], f[d + 1:]
        ok = np.isfinite(fu) & np.isfinite(fd_)
        g = np.where(ok, (np.where(ok, fu, 0.0) - np.where(ok, fd_, 0.0)) / np.maximum(up - dn, 1e-300), 0.0)
        frozen = ((x[b] <= lo) & (g > 0)) | ((x[b] >= hi) & (g < 0))
        pg = np.where(frozen, 0.0, np.abs(g))
        free = up > dn
        bound = GTOL + 2.0 * RTOL_LP * max(1.0, abs(f[0])) / np.where(free, up - dn, 1.0)
        ratio = np.where(free, pg / bound, 0.0)
        worst = max(worst, ratio.max())
        assert np.all(ratio <= 1.0), "start %d: oracle projected gradient %r against %r" % (b, pg, bound)
    print("p=%d q=%d: worst oracle projected gradient / bound %.3e over %d starts" % (p, q, worst, conv.size))


# ---- the multi-series path: a start's result does not depend on what else the call holds ------------------------------------------
def _six_series():
    return [_series(n, seed=200 + i) for i, n in enumerate([80, 31, 64, 100, 47, 72])]


def _ms_problem(cpa, p, q, nt):
    series = _six_series()
    mc = cpa.MultiContext(series, p, q)
    S = len(series)
    which = np.repeat(np.arange(S), nt)
    x0 = np.concatenate([_starts(p, q, t, y, nt, 10 * s + p) for s, (t, y, _) in enumerate(series)])
    boxes = [_box(t, y, e, p, q) for t, y, e in series]
    lo, hi = np.array([b[1] for b in boxes])[which], np.array([b[2] for b in boxes])[which]
    return series, mc, which, x0, lo, hi


@pytest.mark.parametrize("p,q", ORDERS)
def test_ms_result_of_a_start_is_independent_of_the_batch(cpa, p, q):
    """k_logdens_carma_lane_ms gives a point the same bits whatever else the launch holds
    (test_gpu_mseries.py::test_batch_composition_does_not_change_values), and the loop treats a start the same whatever its
    place in the compacted lists: so x, fun, nit and status of a start are bitwise the same among starts of other series, in
    reversed order, and alone.  (nfev is not: alone, more candidates carry their stencil, which saves centre points.)"""
    series, mc, which, x0, lo, hi = _ms_problem(cpa, p, q, 3)
    kw = dict(maxiter=MAXITER, gtol=GTOL, fd_step=FD, ignore_prior=p > 1)
    full = mc.mle_batched(x0, which, lo, hi, **kw)
    assert np.any(full[2] > 5) and len(set(full[2].tolist())) > 3
    rev = mc.mle_batched(x0[::-1], which[::-1], lo[::-1], hi[::-1], **kw)
    for k in (0, 1, 2, 4):
        assert np.array_equal(rev[k][::-1], full[k], equal_nan=True), "reversed order, output %d" % k
    for b in range(0, which.size, 2):
        one = mc.mle_batched(x0[b:b + 1], which[b:b + 1], lo[b:b + 1], hi[b:b + 1], **kw)
        for k in (0, 1, 2, 4):
            assert np.array_equal(one[k][0], full[k][b], equal_nan=True), "start %d alone, output %d" % (b, k)
        assert one[3][0] - one[2][0] <= full[3][b] <= one[3][0] + one[2][0]


@pytest.mark.parametrize("p,q", [(1, 0), (2, 1)])
def test_single_series_result_of_a_start_barely_depends_on_the_batch(cpa, p, q):
    # carma_mle_batched evaluates through carma_logdensity_batch, whose launch shape -- and with it the rounding of a value --
    # depends on the number of points in the launch: a start run alone sees other last bits than in a batch, the searches
    # part in the last digits, and only the optimum they reach can be compared: fun to 1e-6 relative.  (The orders are the two
    # whose surface on this series has one optimum; at (5,3) two searches that part can end in different local optima.)
    P = problem(cpa, p, q)
    t, y, e = P["t"], P["y"], P["e"]
    bnds, _, _ = _box(t, y, e, p, q)
    ctx = cpa.Context(t, y, e, p, q)
    fun = P["runs"]["default"][1]
    for b in range(0, NSTARTS, 4):
        one = ctx.mle_batched(P["x0"][b:b + 1], bnds, maxiter=MAXITER, gtol=GTOL, fd_step=FD, ignore_prior=P["ip"])
        assert abs(one[1][0] - fun[b]) <= 1e-6 * abs(fun[b]), (b, one[1][0], fun[b])


@pytest.mark.parametrize("p,q", [(2, 1), (5, 3)])
def test_ms_every_start_has_its_own_box_and_series(cpa, p, q):
    """Start b: lo = hi in coordinate 1 at a value of its own, a tight box of its own around its start elsewhere, series
    which[b].  The returned coordinate is exactly that value, x lies in b's box, and fun is the oracle's value on series
    which[b] -- not on the neighbouring series, where the value is far away."""
    series, mc, which, x0, lo, hi = _ms_problem(cpa, p, q, 4)
    B, d = x0.shape
    S = len(series)
    x0 = np.clip(x0, lo, hi)
    rng = np.random.default_rng(5)
    w = 0.05 * np.maximum(1.0, np.abs(x0)) * rng.uniform(0.5, 1.5, (B, d))
    lo, hi = np.maximum(lo, x0 - w), np.minimum(hi, x0 + w)
    pin = 0.9 + 0.2 * (np.arange(B) + 0.5) / B              # inside (0.9, 1.1), the error scale's box, one value per start
    lo[:, 1] = hi[:, 1] = pin
    x0[:, 1] = 0.5                                           # outside: projected onto the pinned value
    ip = p > 1
    x, fun, nit, nfev, status = mc.mle_batched(x0, which, lo, hi, maxiter=MAXITER, gtol=GTOL, fd_step=FD, ignore_prior=ip)
    assert np.array_equal(x[:, 1], pin)
    assert np.all(x >= lo) and np.all(x <= hi)
    assert np.any(nit > 5)
    free = np.arange(d) != 1
    print("p=%d q=%d: %d of %d starts end on a face of their own box, nit %d ... %d" % (
        p, q, np.any((x[:, free] == lo[:, free]) | (x[:, free] == hi[:, free]), axis=1).sum(), B, nit.min(), nit.max()))
    for s, (t, y, e) in enumerate(series):
        sel = np.flatnonzero(which == s)
        tt, yy, ee = mc.data(s)
        om = orc.OracleModel(t, y, e, p, q, max_stdev=mc.prior(s)[0])
        # (a prior-like start of CARMA(5,3) can lie where the log-density is not finite: status 4, by the oracle on ITS series)
        dead = ~np.isfinite(_oracle_f(om, np.clip(x0[sel], lo[sel], hi[sel]), ip))
        assert np.array_equal(status[sel] == 4, dead), (s, status[sel], dead)
        assert dead.sum() <= 1
        sel = sel[~dead]
        own = -_oracle_f(om, x[sel], ip)
        arb = (lambda i, sel=sel: loglik_truth(tt, yy, ee, x[sel[i]], p, q)[0]) if p > 1 else None
        assert_parity(-fun[sel], own, RTOL_LP, "own series p=%d q=%d series %d" % (p, q, s), arbiter=arb)
        n = (s + 1) % S
        tn, yn, en = series[n]
        other = _oracle_f(orc.OracleModel(tn, yn, en, p, q, max_stdev=mc.prior(n)[0]), x[sel], ip)
        assert np.all(~(np.abs(fun[sel] - other) <= 1e4 * RTOL_LP * np.abs(fun[sel]))), (s, fun[sel], other)


# ---- status 4 ----------------------------------------------------------------------------------------------------------------------
def test_a_start_without_a_finite_value_is_status_4_and_leaves_the_others_alone(cpa):
    """CARMA(5,3) with the second quadratic factor of the AR polynomial equal to the first: repeated roots, the log-density is
    not finite (test_gpu_parity.py::test_prior_bounds_and_failures).  Through MultiContext.mle_batched, Context.mle_batched and
    CarmaModelSet.get_mle(starts=...)."""
    import carmcmc as cm
    from carma_pack_amd.carma_pack import STATUS_TEXT
    p, q = 5, 3
    t, y, e = _series()
    bnds, lo, hi = _box(t, y, e, p, q)
    good = np.clip(_starts(p, q, t, y, 12, 77), lo, hi)
    om = orc.OracleModel(t, y, e, p, q)
    good = good[np.isfinite(_oracle_f(om, good, True))][:5]
    assert good.shape[0] == 5
    bad = good[0].copy()
    bad[5:7] = bad[3:5]
    assert np.all(bad >= lo) and np.all(bad <= hi) and not np.isfinite(_oracle_f(om, bad[None], True)[0])
    x0 = np.insert(good, 2, bad, axis=0)
    keep = np.arange(6) != 2
    kw = dict(maxiter=MAXITER, gtol=GTOL, fd_step=FD, ignore_prior=True)
    # the multi-series path: values do not depend on the batch, so the other starts are the same bit for bit
    mc = cpa.MultiContext([(t, y, e)], p, q)
    x, fun, nit, nfev, status = mc.mle_batched(x0, 0, lo, hi, **kw)
    ref = mc.mle_batched(good, 0, lo, hi, **kw)
    assert status[2] == 4 and nit[2] == 0 and fun[2] == 1e300 and nfev[2] == 2 * x0.shape[1] + 1 and np.array_equal(x[2], bad)
    assert np.all(status[keep] != 4) and np.all(nit[keep] > 0)
    for k, got in enumerate((x, fun, nit, nfev, status)):
        if k != 3:
            assert np.array_equal(got[keep], ref[k]), "output %d of the other starts changed" % k
    # the single-series entry point
    x1, fun1, nit1, nfev1, status1 = cpa.Context(t, y, e, p, q).mle_batched(x0, bnds, **kw)
    assert status1[2] == 4 and nit1[2] == 0 and fun1[2] == 1e300 and np.array_equal(x1[2], bad)
    assert np.all(status1[keep] != 4) and np.all(fun1[keep] < 1e299)
    # the model classes: not a success, in words, and never the best
    mset = cm.CarmaModelSet([(t, y, e)], p=p, q=q)
    allr = mset.get_mle(p, q, starts=x0[None], return_all=True)[0]
    assert not allr[2].success and allr[2].message == STATUS_TEXT[4] == "no finite value at the start"
    assert allr[2].nit == 0 and allr[2].fun == 1e300
    assert all(r.message != STATUS_TEXT[4] for i, r in enumerate(allr) if i != 2)
    best = mset.get_mle(p, q, starts=x0[None])[0]
    assert best.fun == min(r.fun for i, r in enumerate(allr) if i != 2) and best.fun < 1e299
    # every start infeasible: what is handed out says so
    only = mset.get_mle(p, q, starts=np.stack([bad, bad])[None])[0]
    assert not only.success and only.message == STATUS_TEXT[4]
