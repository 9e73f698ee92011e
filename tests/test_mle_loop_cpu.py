"""CPU-only: the lock-step optimiser's loop itself (carma_pack_amd/csrc/carma_mle_loop.h, the code behind carma_mle_batched and
carma_mle_batched_ms) on objectives whose answers are known, through the host harness tests/mleloop/ (tests/mleloop_ref.py).
The evaluator calls back into numpy and every launch is recorded, so the tests see which points the loop evaluates, for which
start, and in which launch."""
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.optimize import minimize as sp_minimize

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import mleloop_ref as ml  # noqa: E402
from batched_opt_proto import minimize_batched  # noqa: E402
from carma_pack_amd.carma_pack import STATUS_TEXT  # noqa: E402

GTOL, FD = 1e-5, 1e-6
INF = np.inf


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- objectives (all pointwise: the value of a point does not depend on what else the launch holds) ----------------------------
def rowsum(a):
    """Sum over the last axis, left to right, elementwise over the points: the bits of a point's value must not depend on how
    many points share the call (a BLAS product or a blocked reduction may round differently for different shapes)."""
    acc = a[:, 0].copy()
    for j in range(1, a.shape[1]):
        acc += a[:, j]
    return acc


class Quadratic(object):
    """f = 1/2 (x - c)' H (x - c), H = Q diag(lam) Q', lam geometric from 1 to cond, c uniform in [-2, 2]^d; box [-1, 1]^d."""

    def __init__(self, d, cond, seed):
        rng = np.random.default_rng(seed)
        Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        self.d, self.cond = d, cond
        self.lam = np.geomspace(1.0, cond, d) if d > 1 else np.ones(1)
        self.H = (Q * self.lam) @ Q.T
        self.H = 0.5 * (self.H + self.H.T)
        self.c = rng.uniform(-2.0, 2.0, d)
        self.lo, self.hi = -np.ones(d), np.ones(d)
        self.x0 = rng.uniform(-1.5, 1.5, (60, d))          # some outside the box: projected first

    def __call__(self, pts, owner=None):
        r = pts - self.c
        Hr = np.zeros_like(r)
        for j in range(self.d):
            Hr += r[:, j:j + 1] * self.H[j]
        return 0.5 * rowsum(Hr * r)

    def grad(self, x):
        return self.H @ (x - self.c)

    def answer(self):
        """(x*, state): state -1 / +1 on that bound, 0 free.  d <= 5: enumeration of the 3^d active sets (the one that is
        feasible with multipliers of the right sign; strictly convex, so unique).  Larger d: scipy's L-BFGS-B with the analytic
        gradient, run until the projected gradient is below 1e-14."""
        d = self.d
        if d <= 5:
            for code in range(3 ** d):
                st = np.array([(code // 3 ** j) % 3 - 1 for j in range(d)])
                fr = st == 0
                x = st.astype(float)
                if fr.any():
                    rhs = -self.H[np.ix_(fr, ~fr)] @ (x[~fr] - self.c[~fr])
                    x[fr] = self.c[fr] + np.linalg.solve(self.H[np.ix_(fr, fr)], rhs)
                g = self.grad(x)
                if np.all(np.abs(x[fr]) < 1.0) and np.all(g[st < 0] > 0) and np.all(g[st > 0] < 0):
                    return x, st
            raise AssertionError("no active set satisfies the optimality conditions")
        r = sp_minimize(lambda v: (float(self(v[None])[0]), self.grad(v)), np.zeros(d), jac=True, method="L-BFGS-B",
                        bounds=[(-1.0, 1.0)] * d, options=dict(gtol=1e-14, ftol=0.0, maxiter=100000, maxfun=1000000, maxcor=30))
        st = np.where(r.x <= -1.0, -1, np.where(r.x >= 1.0, 1, 0))
        # scipy stops where its own arithmetic stalls (a projected gradient of some 1e-9 here); on the active set it found the
        # free variables solve a linear system, which is then solved directly and must satisfy the optimality conditions
        fr = st == 0
        x = st.astype(float)
        x[fr] = self.c[fr] + np.linalg.solve(self.H[np.ix_(fr, fr)], -self.H[np.ix_(fr, ~fr)] @ (x[~fr] - self.c[~fr]))
        g = self.grad(x)
        assert np.abs(x - r.x).max() < 1e-7 and np.all(np.abs(x[fr]) < 1.0) and np.all(g[st < 0] > 0) and np.all(g[st > 0] < 0)
        return x, st


QUADS = [(d, cond) for d in (1, 3, 5, 16) for cond in (1, 100)]
_quads = {}


def quad(d, cond):
    """The problem, its answer and the harness's run from its 60 starts (ftol = 0: only the gradient rule can end a start);
    computed once and shared."""
    if (d, cond) not in _quads:
        q = Quadratic(d, cond, 1000 * d + cond)
        xs, st = q.answer()
        run = ml.minimize(q, q.x0, q.lo, q.hi, ftol=0.0, gtol=GTOL, fd_step=FD)
        for a in (xs, st, run.x, run.fun, run.nit, run.nfev, run.status):
            a.setflags(write=False)
        _quads[(d, cond)] = (q, xs, st, run)
    return _quads[(d, cond)]


def answer_bound(d, fmax, lam_min, x):
    """||x - x*||_2 over the free variables <= sqrt(d) (gtol + delta) / lam_min.  Derived, not tuned: at status 0 every free
    component of the difference quotient is within gtol; the central difference of a quadratic is its gradient up to the
    rounding of the two values it subtracts, delta = 4 eps max|f| / (2 fd_step max(1, |x|)) (the coordinate with the smallest
    step decides); and ||x - x*|| <= ||g|| / lam_min on the free subspace."""
    xs = np.maximum(1.0, np.abs(x)).min()
    return np.sqrt(d) * (GTOL + 4.0 * ml.EPS * fmax / (2.0 * FD * xs)) / lam_min


def rosen(pts, owner=None):
    return rowsum(100.0 * (pts[:, 1:] - pts[:, :-1] ** 2) ** 2 + (1.0 - pts[:, :-1]) ** 2)


def rosen_starts(d, B=60):
    return np.random.default_rng(50 + d).uniform(-1.5, 1.5, (B, d))


def infeasible_region(pts, owner=None):
    """The problem of test_batched_opt.py: minimum outside the box, NaN beyond x_0 < -0.5."""
    v = rowsum((pts - 3.0) ** 2)
    v[pts[:, 0] < -0.5] = np.nan
    return v


INFEASIBLE_BOX = (np.array([-1.0, -INF, 0.0]), np.array([1.0, INF, 2.5]))


# ---- the harness and the stand-alone program ---------------------------------------------------------------------------------
def test_constants_are_the_documented_ones():
    assert ml.constants() == (1e300, 8, 3)


def test_stand_alone_program_meets_every_case():
    """tests/mleloop/mleloop_main.cpp: the quadratic, clip, kink and memory cases with built-in evaluators, no Python between
    the loop and the objective.  Built and run here WITHOUT sanitizers (a sanitizer build of it is a matter for the command
    line)."""
    r = subprocess.run([ml.build_main()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "all cases met" in r.stdout


# ---- box-constrained convex quadratics ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,cond", QUADS)
def test_quadratic_in_a_box_reaches_the_exact_answer(d, cond):
    q, xs, st, run = quad(d, cond)
    assert (st != 0).any() or d == 1, "no bound is active: the problem does not test the projection"
    assert np.all(run.status == 0), (run.status, run.nit)
    fmax = run.fmax()
    worst = 0.0
    for b in range(run.x.shape[0]):
        x = run.x[b]
        assert np.array_equal(x[st != 0], st[st != 0].astype(float)), "start %d: active set differs from the reference's" % b
        assert np.all(np.abs(x[st == 0]) < 1.0), "start %d: a free variable sits on a bound" % b
        err = np.linalg.norm(x[st == 0] - xs[st == 0])
        bound = answer_bound(d, fmax, 1.0, x)
        worst = max(worst, err / bound)
        assert err <= bound, "start %d: %.3e from the answer, bound %.3e" % (b, err, bound)
        assert run.fun[b] == q(x[None])[0]
    print("quadratic d=%d cond=%d: nit <= %d, worst distance / bound %.3f (bound %.2e)" % (d, cond, run.nit.max(), worst, bound))


# ---- every start its own problem in its own box ----------------------------------------------------------------------------------
class Separable(object):
    """Start b minimises sum_j w_bj (x_j - c_bj)^2 in [lo_b, hi_b]; the answer is clip(c_b, lo_b, hi_b).  The scale of w_b is
    spread over four decades, so the starts finish at very different iterations.  Boxes by b mod 5: lo = hi in one coordinate,
    one-sided (no lower bound / no upper bound), wholly infinite, finite."""

    def __init__(self, B, d=3, seed=0):
        rng = np.random.default_rng(seed)
        self.B, self.d = B, d
        scale = 10.0 ** np.linspace(-2.0, 2.0, B)[rng.permutation(B)] if B > 1 else np.ones(1)
        self.w = scale[:, None] * rng.uniform(1.0, 4.0, (B, d))
        off = np.arange(B)[:, None].astype(float)
        self.c = off + rng.uniform(-2.0, 2.0, (B, d))
        self.lo = off + rng.uniform(-1.5, -0.1, (B, d))
        self.hi = off + rng.uniform(0.1, 1.5, (B, d))
        self.pinned = np.full(B, -1)
        for b in range(B):
            kind = b % 5
            if kind == 0:
                self.pinned[b] = b % d
                self.hi[b, b % d] = self.lo[b, b % d] = b + 0.1 + 0.01 * b
            elif kind == 1:
                self.lo[b, (b + 1) % d] = -INF
            elif kind == 2:
                self.hi[b, (b + 2) % d] = INF
            elif kind == 3:
                self.lo[b], self.hi[b] = -INF, INF
        # every start begins strictly inside its box (where it has an interior) and away from its answer, so that all B of them
        # share the first line-search launch: B is then the number KS is computed from
        inside = np.where(np.isfinite(self.lo), self.lo, off - 1.5) + rng.uniform(0.2, 0.8, (B, d)) * (
            np.where(np.isfinite(self.hi), self.hi, off + 1.5) - np.where(np.isfinite(self.lo), self.lo, off - 1.5))
        self.x0 = np.where(np.abs(inside - np.clip(self.c, self.lo, self.hi)) > 0.05, inside, inside + 0.07)
        self.x0 = np.where(self.lo == self.hi, self.x0 + 3.0, self.x0)          # the pinned coordinate starts outside: projected

    def __call__(self, pts, owner):
        return rowsum(self.w[owner] * (pts - self.c[owner]) ** 2)

    def alone(self, b):
        """Start b as a problem of its own (owner 0 is start b)."""
        return lambda pts, owner: rowsum(self.w[b] * (pts - self.c[b]) ** 2)


@pytest.mark.parametrize("B", [1, 18, 19, 52, 60])
def test_every_start_its_own_problem_and_box(B):
    d = 3
    p = Separable(B, d, seed=B)
    run = ml.minimize(p, p.x0, p.lo, p.hi, per_start=True, ftol=0.0, gtol=GTOL, fd_step=FD)
    assert np.all(run.status == 0), run.status
    want = np.clip(p.c, p.lo, p.hi)
    worst = 0.0
    fmax = np.zeros(B)
    for pts, owner, v in run.calls:
        np.maximum.at(fmax, owner, np.abs(v))
    for b in range(B):
        onb = (want[b] == p.lo[b]) | (want[b] == p.hi[b])
        assert np.array_equal(run.x[b, onb], want[b, onb]), "start %d: not on its own bounds" % b
        if p.pinned[b] >= 0:
            assert run.x[b, p.pinned[b]] == p.lo[b, p.pinned[b]]                  # exactly that number
        err = np.linalg.norm(run.x[b, ~onb] - want[b, ~onb])
        bound = answer_bound(d, fmax[b], 2.0 * p.w[b].min(), run.x[b])
        worst = max(worst, err / bound)
        assert err <= bound, "start %d: %.3e from clip(c, lo, hi), bound %.3e" % (b, err, bound)
    if B > 1:
        assert run.nit.max() >= 2 * max(run.nit.min(), 1), "the starts do not finish at different iterations: %s" % run.nit
    # ---- what the recorded launches show
    alone = []
    for b in range(B):
        r1 = ml.minimize(p.alone(b), p.x0[b:b + 1], p.lo[b:b + 1], p.hi[b:b + 1], per_start=True, ftol=0.0, gtol=GTOL, fd_step=FD)
        assert same_bits(r1.x[0], run.x[b]) and same_bits(r1.fun, run.fun[b:b + 1]), "start %d alone gives other bits" % b
        assert r1.nit[0] == run.nit[b] and r1.status[0] == run.status[b]
        alone.append(set(pt.tobytes() for pts, _, _ in r1.calls for pt in pts))
    for n, (pts, owner, v) in enumerate(run.calls):
        assert owner.min() >= 0 and owner.max() < B
        # every evaluated point lies in its owner's box
        assert np.all(pts >= p.lo[owner]) and np.all(pts <= p.hi[owner]), "launch %d evaluates a point outside its owner's box" % n
        # and belongs to its owner's iterates: run alone (one start: every candidate of the first round carries its stencil),
        # that start evaluates a superset of the points it is evaluated at in any batch
        for k in range(owner.size):
            assert pts[k].tobytes() in alone[owner[k]], "launch %d point %d is none of start %d's" % (n, k, owner[k])
    first, iters = ml.parse_calls(run, d)
    assert np.array_equal(first, np.arange(B))
    seen = np.zeros(B, dtype=int)                            # iterations each start took part in
    ks = set()
    for it, rec in enumerate(iters):
        assert len(rec["ls"]) <= 4, "iteration %d: %d line-search rounds" % (it, len(rec["ls"]))
        ks.add(ml.ks_of(rec["ls"][0].size, d))
        for a, bnext in zip(rec["ls"][:-1], rec["ls"][1:]):
            assert np.all(np.isin(bnext, a)), "iteration %d: a later round holds a start the round before did not" % it
        if rec["grad"] is not None:
            assert np.all(np.isin(rec["grad"], rec["ls"][0]))
        # no start is evaluated after the iteration in which it stopped: all took part from iteration 0 on without a gap
        assert np.all(seen[rec["ls"][0]] == it), "iteration %d holds a start that had stopped" % it
        seen[rec["ls"][0]] += 1
    assert np.array_equal(seen, run.nit), "iterations seen in the launches %s, reported %s" % (seen, run.nit)
    if B == 60:
        assert {1, 8} <= ks, "KS took the values %s: the run does not cross both thresholds" % sorted(ks)
    # all B starts share the first line-search launch: either side of where KS leaves 8 and reaches 1
    assert iters[0]["ls"][0].size == B and ml.ks_of(B, d) == {1: 8, 18: 8, 19: 7, 52: 1, 60: 1}[B]
    print("separable B=%d: nit %d ... %d, KS values %s, worst distance / bound %.3f" % (B, run.nit.min(), run.nit.max(), sorted(ks), worst))


# ---- the lock-step machinery is transparent --------------------------------------------------------------------------------------
def _transparent(fun, x0, lo, hi, other, other_x0, maxiter, what):
    """Start b's x, fun, nit and status are bitwise the same run alone, in the batch, in the batch reversed and among starts of
    another problem (`other`, per-start evaluator, a box per start); nfev differs only by the centre points the speculative
    stencil saves."""
    B, d = x0.shape
    kw = dict(ftol=0.0, gtol=GTOL, fd_step=FD, maxiter=maxiter)
    batch = ml.minimize(fun, x0, lo, hi, **kw)
    rev = ml.minimize(fun, x0[::-1], lo, hi, **kw)
    mixed_x0 = np.empty((2 * B, d))
    mixed_x0[0::2], mixed_x0[1::2] = other_x0[:B], x0
    mine = np.arange(2 * B) % 2 == 1

    def mixed_fun(pts, owner):
        out = np.empty(owner.size)
        m = mine[owner]
        out[m] = fun(pts[m])
        out[~m] = other(pts[~m])
        return out
    mixed = ml.minimize(mixed_fun, mixed_x0, np.tile(lo, (2 * B, 1)), np.tile(hi, (2 * B, 1)), per_start=True, **kw)
    for name, r, sel in (("reversed", rev, slice(None, None, -1)), ("among other problems", mixed, slice(1, None, 2))):
        assert same_bits(r.x[sel], batch.x) and same_bits(r.fun[sel], batch.fun), "%s, %s: other bits than in the batch" % (what, name)
        assert np.array_equal(r.nit[sel], batch.nit) and np.array_equal(r.status[sel], batch.status), (what, name)
    for b in range(B):
        one = ml.minimize(fun, x0[b:b + 1], lo, hi, **kw)
        assert same_bits(one.x[0], batch.x[b]) and same_bits(one.fun, batch.fun[b:b + 1]), "%s: start %d alone gives other bits" % (what, b)
        assert one.nit[0] == batch.nit[b] and one.status[0] == batch.status[b], (what, b)
        for r, i in ((batch, b), (rev, B - 1 - b), (mixed, 2 * b + 1)):
            assert one.nfev[0] - one.nit[0] <= r.nfev[i] <= one.nfev[0] + one.nit[0], (what, b, one.nfev[0], r.nfev[i], one.nit[0])
    return batch


@pytest.mark.parametrize("d", [2, 4])
def test_batching_is_transparent_on_rosenbrock(d):
    x0 = rosen_starts(d)
    q = Quadratic(d, 100, 7)
    lo, hi = np.full(d, -2.0), np.full(d, 2.0)
    batch = _transparent(rosen, x0, lo, hi, q, q.x0, 500, "rosenbrock d=%d" % d)
    assert batch.nit.max() > 30 and len(set(batch.nit.tolist())) > 10          # the starts drop out one by one
    print("rosenbrock d=%d: nit %d ... %d, status counts %s" % (d, batch.nit.min(), batch.nit.max(), np.bincount(batch.status, minlength=5)))


@pytest.mark.parametrize("d,cond", [(3, 100), (5, 100), (16, 100)])
def test_batching_is_transparent_on_quadratics(d, cond):
    q, _, _, run = quad(d, cond)
    batch = _transparent(q, q.x0, q.lo, q.hi, rosen if d > 1 else q, rosen_starts(d), 2000, "quadratic d=%d" % d)
    assert same_bits(batch.x, run.x)


# ---- against the prototype ------------------------------------------------------------------------------------------------------
def _proto_problems():
    out = [("quadratic d=%d cond=%d" % (d, c), quad(d, c)[0], quad(d, c)[0].x0[:24], quad(d, c)[0].lo, quad(d, c)[0].hi, 0.0, 2000)
           for d, c in QUADS]
    out.append(("rosenbrock d=4", rosen, rosen_starts(4, 24), np.full(4, -2.0), np.full(4, 2.0), ml.FTOL_DEFAULT, 500))
    x0 = np.zeros((5, 3))
    x0[1] = [0.5, -4.0, 1.0]
    x0[2] = [-0.4, 10.0, 3.0]
    x0[3] = [-0.8, 0.0, 1.0]                                # starts inside the non-finite region: status 4 on both sides
    out.append(("infeasible region", infeasible_region, x0, INFEASIBLE_BOX[0], INFEASIBLE_BOX[1], ml.FTOL_DEFAULT, 2000))
    return out


@pytest.mark.parametrize("mem", [1, 2, 8, 64])
def test_same_searches_as_the_prototype(mem):
    """tests/tools/batched_opt_proto.py is the same algorithm without the speculative stencil, the per-start boxes and the
    compaction by hand: from the same starts, on the same callback, the same searches.  Both sides are deterministic."""
    for what, fun, x0, lo, hi, ftol, maxiter in _proto_problems():
        run = ml.minimize(fun, x0, lo, hi, mem=mem, ftol=ftol, gtol=GTOL, fd_step=FD, maxiter=maxiter)
        bounds = [(None if not np.isfinite(a) else a, None if not np.isfinite(b) else b) for a, b in zip(lo, hi)]
        with np.errstate(all="ignore"):
            ref = minimize_batched(lambda pts: fun(pts), x0, bounds, maxiter=maxiter, m=mem, ftol=ftol, gtol=GTOL, fd_step=FD)
        if mem <= 2 and what.startswith(("quadratic d=5 cond=100", "quadratic d=16 cond=100", "rosenbrock")):
            assert run.nit.max() > mem + 1                  # more iterations than pairs: the oldest pair is dropped
        for b, r in enumerate(ref):
            tag = "%s, mem %d, start %d" % (what, mem, b)
            assert STATUS_TEXT[run.status[b]] == r.message, "%s: %s against the prototype's %s" % (tag, STATUS_TEXT[run.status[b]], r.message)
            assert run.nit[b] == r.nit, "%s: nit %d against the prototype's %d" % (tag, run.nit[b], r.nit)
            assert np.all(np.abs(run.x[b] - r.x) <= 1e-8 * np.maximum(1.0, np.abs(r.x))), "%s: x %r against %r" % (tag, run.x[b], r.x)
            assert abs(run.fun[b] - r.fun) <= 1e-8 * max(1.0, abs(r.fun)), "%s: fun %r against %r" % (tag, run.fun[b], r.fun)
            assert r.nfev - r.nit <= run.nfev[b] <= r.nfev, "%s: nfev %d against the prototype's %d (nit %d)" % (tag, run.nfev[b], r.nfev, r.nit)
            assert (run.status[b] < 2) == r.success


# ---- stopping rules and edges ---------------------------------------------------------------------------------------------------
def test_maxiter_ends_a_start_with_status_2():
    x0 = rosen_starts(4, 7)
    run = ml.minimize(rosen, x0, np.full(4, -2.0), np.full(4, 2.0), maxiter=3)
    assert np.all(run.status == 2) and np.all(run.nit == 3)


def test_maxiter_zero_returns_the_projected_start():
    x0 = np.array([[3.0, -0.5, 0.25, -7.0], [0.1, 0.2, 0.3, 0.4]])
    lo, hi = np.full(4, -2.0), np.array([2.0, 2.0, INF, 2.0])
    run = ml.minimize(rosen, x0, lo, hi, maxiter=0)
    want = np.clip(x0, lo, hi)
    assert same_bits(run.x, want) and same_bits(run.fun, rosen(want))
    assert np.all(run.nit == 0) and np.all(run.status == 2) and np.all(run.nfev == 9)
    assert len(run.calls) == 1 and same_bits(run.calls[0][0][[0, 9]], want)      # a start outside the box is projected first


def test_no_starts():
    for per_start in (False, True):
        run = ml.minimize(rosen, np.empty((0, 4)), np.full(4, -2.0), np.full(4, 2.0), per_start=per_start)
        assert run.x.shape == (0, 4) and run.fun.size == 0 and run.calls == []


def test_kink_ends_with_a_failed_line_search():
    """f = sum |x - x0| + (x - x0)_0 / 2: the central difference at x0 says downhill along coordinate 0, but every step goes
    up.  32 step lengths in four rounds, then status 3 at x0."""
    d = 3
    x0 = np.array([[0.3, -0.7, 1.1]])
    run = ml.minimize(lambda pts, o: rowsum(np.abs(pts - x0)) + 0.5 * (pts[:, 0] - x0[0, 0]), x0, np.full(d, -INF), np.full(d, INF),
                      per_start=True, ftol=0.0)
    assert run.status[0] == 3 and run.nit[0] == 0 and run.nfev[0] == 2 * d + 1 + 32
    assert same_bits(run.x, x0) and run.fun[0] == 0.0
    _, iters = ml.parse_calls(run, d)
    assert len(iters) == 1 and len(iters[0]["ls"]) == 4 and iters[0]["grad"] is None


def test_second_round_of_the_line_search():
    """f = 1/2 10^6 ||x||^2 from ||x0|| = 10^-3: the first step is of unit length, so the eight step lengths 1 ... 2^-7 of the
    first round all overshoot and the second round (from 2^-8 on) is taken."""
    d = 3
    x0 = np.array([[6e-4, -8e-4, 0.0]])
    run = ml.minimize(lambda pts, o: 0.5e6 * rowsum(pts * pts), x0, np.full(d, -INF), np.full(d, INF), per_start=True, ftol=0.0)
    _, iters = ml.parse_calls(run, d)
    assert len(iters[0]["ls"]) == 2
    assert run.status[0] == 0
    assert np.linalg.norm(run.x[0]) <= answer_bound(d, run.fmax(), 1e6, run.x[0])


def _ball(pts, owner=None):
    """sum (x - c)^2 with the unit ball around the origin non-finite."""
    v = rowsum((pts - np.array([3.0, 2.0, -1.0])) ** 2)
    v[rowsum(pts * pts) < 1.0] = np.nan
    return v


def test_start_in_a_non_finite_region_is_status_4():
    d = 3
    lo, hi = np.full(d, -5.0), np.full(d, 5.0)
    rng = np.random.default_rng(4)
    x0 = np.insert(rng.uniform(2.0, 4.0, (7, d)), 4, [0.2, -0.3, 0.4], axis=0)          # start 4 inside the ball
    run = ml.minimize(_ball, x0, lo, hi)
    ref = ml.minimize(_ball, np.delete(x0, 4, axis=0), lo, hi)
    assert run.status[4] == 4 and run.nit[4] == 0 and run.fun[4] == 1e300 and run.nfev[4] == 2 * d + 1
    assert same_bits(run.x[4], x0[4])
    keep = np.arange(8) != 4
    assert np.all(run.status[keep] < 2)
    for got, want in ((run.x[keep], ref.x), (run.fun[keep], ref.fun)):
        assert same_bits(got, want)                          # the other starts are not affected
    assert np.array_equal(run.nit[keep], ref.nit) and np.array_equal(run.status[keep], ref.status)
    # the start is evaluated once, in the first launch, and never again
    assert all(not np.any(np.all(pts == x0[4], axis=1)) for pts, _, _ in run.calls[1:])
    # a start OUTSIDE the box whose projection is infeasible, and maxiter = 0: status 4 as well, x the projected start
    far = np.array([[0.2, 0.1, -9.0]])
    r0 = ml.minimize(_ball, far, np.full(d, -0.5), np.full(d, 0.5), maxiter=0)
    assert r0.status[0] == 4 and same_bits(r0.x, [[0.2, 0.1, -0.5]]) and r0.fun[0] == 1e300 and r0.nit[0] == 0
    assert STATUS_TEXT[4] == "no finite value at the start"


def test_start_next_to_a_non_finite_region_converges():
    """x0 sits 5e-7 outside the ball: the lower stencil point of coordinate 0 is inside, so that component of g is 0 and the
    first steps run along the other coordinates, away from the ball; the start still reaches the minimiser."""
    d = 3
    x0 = np.array([[1.0 + 5e-7, 0.0, 0.0]])
    run = ml.minimize(_ball, x0, np.full(d, -5.0), np.full(d, 5.0), ftol=0.0)
    pts, _, v = run.calls[0]
    assert np.isfinite(v[0]) and not np.isfinite(v[1 + d]) and np.isfinite(np.delete(v, 1 + d)).all()
    # the first step leaves coordinate 0 where it is: its component of g was 0
    first_round = run.calls[1][0][:8]
    assert np.all(first_round[:, 0] == x0[0, 0]) and np.all(first_round[:, 1] > 0.0)
    assert run.status[0] == 0
    assert np.linalg.norm(run.x[0] - [3.0, 2.0, -1.0]) <= answer_bound(d, run.fmax(), 2.0, run.x[0])


def _valley(pts, owner=None):
    """A valley with a flat (quartic) bottom on a plateau: down the wall the iterations are large, along the bottom the
    quasi-Newton steps converge only linearly and the decrease per iteration falls below ftol |f| while the gradient is still
    above gtol."""
    return 100.0 + 0.5 * pts[:, 0] ** 2 + 0.01 * pts[:, 1] ** 4


def test_ftol_ends_a_start_only_after_a_restart_and_three_small_iterations():
    d = 2
    x0 = np.array([[1.0, 1.0]])
    lo, hi = np.full(d, -INF), np.full(d, INF)
    ftol = ml.FTOL_DEFAULT
    run = ml.minimize(_valley, x0, lo, hi, per_start=True, ftol=ftol, gtol=GTOL)
    assert run.status[0] == 1
    _, iters = ml.parse_calls(run, d)
    assert len(iters) == run.nit[0]                          # the last iteration the launches show is the one that stopped it
    # f after k iterations: the same run cut off at k (the loop is deterministic)
    f = [ml.minimize(_valley, x0, lo, hi, per_start=True, ftol=ftol, gtol=GTOL, maxiter=k).fun[0] for k in range(run.nit[0] + 1)]
    assert f[-1] == run.fun[0]
    small = [(a - b) / max(abs(a), abs(b), 1.0) <= ftol for a, b in zip(f[:-1], f[1:])]
    # the rule, restated: the first small iteration restarts the memory and does not count; three in a row after it end the start
    restarted, nsmall, stop = False, 0, None
    for k, s in enumerate(small):
        nsmall = nsmall + 1 if s else 0
        if s and not restarted:
            restarted, nsmall = True, 0
        if nsmall >= 3:
            stop = k + 1
            break
    assert stop == run.nit[0] == len(small), (small, run.nit[0])
    assert not small[0] and sum(small) >= 4, small          # large iterations first, then the restart and three that count
