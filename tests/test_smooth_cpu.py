"""CPU-only: the one-pass smoother (carma_smooth_carma / _car1) as far as it goes without a device -- the numpy restatement
tests/smooth_ref.py against the 50-digit conditional (mp_truth), the host-only planner carma_smooth_plan.h through the stand-alone
program tests/smooth/plan_main.cpp, the device functions smooth_forward / smooth_backward / smooth_car1 on the CPU lane emulator
(tests/emu/emu_smooth.cpp) against the restatement, and the argument checks of the C entry points, which come before any
device work."""
import ctypes as C
import re

import numpy as np
import pytest

import smooth_build as sb
import smooth_ref as sr
from helpers import irregular_series, model_ma, model_roots
from mp_truth import predict_truth, predict_truth_car1

EINVAL = -22


def _model(p, seed=0):
    rng = np.random.default_rng(7000 + 10 * p + seed)
    return model_roots(rng, p, "mixed" if p > 2 else "complex"), model_ma(rng, p, p - 1)


def _case(p, n, seed=0):
    roots, ma = _model(p, seed)
    t, y, yerr = irregular_series(n, 300 + p + seed)
    y = y - y.mean()
    v1 = sr.model_consts(1.0, roots, ma)[3]
    rng = np.random.default_rng(p + seed)
    tp = np.r_[t[0] - 5000.0, t[0] - 2.5, t[0], t[1], t[7], 0.5 * (t[3] + t[4]), t[-1], t[-1] + 1.5, t[-1] + 5000.0, t[7],
               rng.uniform(t[0] - 8.0, t[-1] + 8.0, 8)]
    return t, y, yerr, float(np.var(y) / v1), roots, ma, rng.permutation(tp)


def _rel(m, v, tm, tv):
    return float(np.max(np.abs(m - tm) / np.maximum(np.abs(tm), np.sqrt(tv)))), float(np.max(np.abs(v - tv) / tv))


# ---- the restatement against the exact conditional ----------------------------------------------------------------------
@pytest.mark.parametrize("p", (2, 5, 7))
def test_restatement_against_the_exact_conditional(p):
    t, y, yerr, sigsqr, roots, ma, tp = _case(p, 48)
    tm, tv = predict_truth(t, y, yerr, sigsqr, roots, ma, tp)
    m, v = sr.smooth_carma(t, y, yerr, sigsqr, roots, ma, tp)
    em, ev = _rel(m, v, tm, tv)
    print("restatement p=%d: mean %.2e, var %.2e from the 50-digit value" % (p, em, ev))
    assert em <= 1e-9 and ev <= 1e-9, (p, em, ev)
    # mu is subtracted from the data and added back to the mean
    m2, v2 = sr.smooth_carma(t, y + 3.25, yerr, sigsqr, roots, ma, tp, mu=3.25)
    assert np.allclose(m2 - 3.25, m, rtol=0, atol=1e-12 * np.sqrt(tv).max()) and np.array_equal(v2, v)


def test_restatement_car1_against_the_exact_conditional():
    t, y, yerr = irregular_series(48, 31)
    y = y - y.mean()
    tp = np.r_[t[0] - 4000.0, t[0] - 3.0, t[0], t[5], t[-1], 0.5 * (t[8] + t[9]), t[-1] + 2.0, t[5], t[-1] + 4000.0]
    for omega in (0.04, 0.7):
        sigsqr = 2.0 * omega * np.var(y)
        tm, tv = predict_truth_car1(t, y, yerr, sigsqr, omega, tp)
        em, ev = _rel(*sr.smooth_car1(t, y, yerr, sigsqr, omega, tp), tm, tv)
        assert em <= 1e-9 and ev <= 1e-9, (omega, em, ev)


def test_band_moments_are_the_mixture_moments():
    rng = np.random.default_rng(5)
    m, v = rng.normal(size=(6, 4)), rng.uniform(0.5, 2.0, (6, 4))
    bm, bv, _, _ = sr.band_moments(m, v)
    # E[x] and Var[x] of the equal-weight mixture, from its raw moments
    assert np.allclose(bm, m.mean(axis=0)) and np.allclose(bv, (v + m ** 2).mean(axis=0) - m.mean(axis=0) ** 2)
    keep = np.array([1, 1, 0, 1, 1, 1], bool)
    assert np.allclose(sr.band_moments(m, v, keep)[0], m[keep].mean(axis=0))
    one = sr.band_moments(m[:1], v[:1])
    assert np.array_equal(one[0], m[0]) and np.array_equal(one[1], v[0])


# ---- the planner header, compiled stand-alone -----------------------------------------------------------------------------
T8 = np.array([0.0, 1.5, 2.0, 4.25, 7.0, 7.5, 11.0, 12.0])
GRID_CASES = {
    "times equal to data times": (T8, T8[[2, 0, 7, 2]]),
    "repeated and unsorted": (T8, np.array([5.0, -1.0, 5.0, 13.0, 3.0, -1.0, 4.25])),
    "M = 0": (T8, np.array([])),
    "M = 1": (T8, np.array([3.0])),
    "M = 2": (T8, np.array([20.0, -20.0])),
    "M = 3": (T8, np.array([7.0, 7.0, 7.25])),
    "n = 1": (T8[:1], np.array([0.0, -1.0, 1.0])),
    "n = 1, M = 0": (T8[:1], np.array([])),
}


@pytest.mark.parametrize("case", sorted(GRID_CASES))
def test_plan_grid_is_the_restatements(case):
    t, tout = GRID_CASES[case]
    grid, dpos, spos, src = sb.plan_merge(t, tout)
    rg, rd, rs, rsrc = sr.merged_grid(t, tout)
    assert np.array_equal(grid, rg) and np.array_equal(dpos, rd) and np.array_equal(spos, rs) and np.array_equal(src, rsrc), case
    # ... and is a grid: ascending, every datum and every requested time exactly once, at its own time
    assert np.all(np.diff(grid) >= 0) and grid.size == t.size + tout.size
    assert np.array_equal(grid[dpos], t) and np.array_equal(grid[spos], tout)
    assert sorted(np.r_[dpos, spos].tolist()) == list(range(grid.size))
    assert np.array_equal(src[dpos], np.arange(t.size)) and np.array_equal(src[spos], -1 - np.arange(tout.size))


@pytest.mark.parametrize("G", (0, 2, 4, 8))
def test_plan_chunks(G):
    E = 64 // G if G else 64
    per_wave = lambda ng: ng * (64 * 32 + E * 32) if G else ng * 64 * 40          # noqa: E731
    ng = 295
    for K in (1, E - 1, E, E + 1, 3 * E + 1, 5000):
        for forced in (1, 2, 0):
            c = sb.plan_chunks(G, ng, K, forced)
            assert c["E"] == E
            assert c["models"] == (min(forced, K) if forced else min(K, ((256 << 20) // per_wave(ng)) * E)), (G, K, forced, c)
            assert c["waves"] == -(-c["models"] // E)
            assert c["bytes"] == c["waves"] * per_wave(ng)
            if G:
                assert c["rec_elems"] == c["waves"] * ng * 64 and c["grp_elems"] == c["waves"] * ng * E
                # 32 G + 32 bytes per point and model when the waves are full
                assert c["bytes"] == c["waves"] * E * ng * (32 * G + 32)
            else:
                assert c["rec_elems"] == c["waves"] * 64 * ng * 5 and c["grp_elems"] == 0
    # automatic: whole waves under the cap, one wave at least however long the grid
    big = sb.plan_chunks(G, 20000, 10 ** 6, 0)
    assert big["models"] % E == 0 and big["bytes"] <= (256 << 20) and big["bytes"] + per_wave(20000) > (256 << 20)
    huge = sb.plan_chunks(G, 4 * 10 ** 6, 100, 0)
    assert huge["waves"] == 1 and huge["models"] == min(100, E)


# ---- the device functions on the lane emulator ------------------------------------------------------------------------------
# Both sides are the same formulas in doubles and differ in summation order, fused multiply-adds and the exponential; the
# restatement itself is 1e-13 ... 1e-12 from the exact value on these inputs (printed by the test above).
EMU_RTOL = 1e-11


@pytest.mark.parametrize("p", (2, 3, 5, 7))
def test_device_functions_on_the_lane_emulator(p):
    t, y, yerr, sigsqr, roots, ma, tp = _case(p, 24, seed=1)
    for mu in (0.0, -1.75):
        rm, rv = sr.smooth_carma(t, y + mu, yerr, sigsqr, roots, ma, tp, mu=mu)
        m, v = sb.smooth_carma(t, y + mu, yerr, sigsqr, roots, ma, tp, mu=mu)
        sc = np.maximum(np.abs(rm - mu), np.sqrt(rv))
        em, ev = float(np.max(np.abs(m - rm) / sc)), float(np.max(np.abs(v - rv) / rv))
        print("emulator p=%d mu=%g: mean %.2e, var %.2e from the restatement" % (p, mu, em, ev))
        assert em <= EMU_RTOL and ev <= EMU_RTOL, (p, mu, em, ev)
    # a repeated time: the same bits wherever it sits
    i = np.flatnonzero(tp == t[7])
    assert i.size == 2 and m[i[0]] == m[i[1]] and v[i[0]] == v[i[1]]


def test_car1_on_the_cpu():
    t, y, yerr = irregular_series(24, 31)
    y = y - y.mean()
    tp = np.r_[t[0] - 4000.0, t[0] - 3.0, t[0], t[5], t[-1], 0.5 * (t[8] + t[9]), t[-1] + 2.0, t[5], t[-1] + 4000.0]
    for omega in (0.04, 0.7):
        sigsqr = 2.0 * omega * np.var(y)
        rm, rv = sr.smooth_car1(t, y, yerr, sigsqr, omega, tp)
        m, v = sb.smooth_car1(t, y, yerr, sigsqr, omega, tp)
        assert np.max(np.abs(m - rm) / np.maximum(np.abs(rm), np.sqrt(rv))) <= EMU_RTOL and np.max(np.abs(v - rv) / rv) <= EMU_RTOL


# ---- the C entry points: symbols and argument errors (before any device work) -------------------------------------------------
def _lib():
    import carma_pack_amd._lib as L
    return L


def test_symbols_exported_declared_and_listed():
    import os
    L = _lib()
    txt = open(os.path.join(sb.ROOT, "include", "carma_mi355.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    dll = C.CDLL(L.LIB_PATH)
    for s in ("carma_smooth_carma", "carma_smooth_car1", "carma_msmooth"):
        assert hasattr(dll, s)
        assert re.search(r"\b%s\s*\(" % s, txt), "%s is not declared in the header" % s
        assert s in L.EXPORTS
        assert getattr(L.lib, s).argtypes is not None


GOOD = np.array([[-0.1 - 0.5j, -0.1 + 0.5j, -0.3]] * 3)


def test_argument_errors_name_the_model_and_come_before_device_work():
    L = _lib()
    t, y, e = irregular_series(20, 5)
    ts = np.linspace(t[0], t[-1], 7)
    sig, ma = np.ones(3), np.ones((3, 1))
    bad = GOOD.copy()
    bad[1, 1] = -0.1 + 0.4j
    with pytest.raises(ValueError, match="model 1.*conjugate"):
        L.smooth_carma(t, y, e, sig, bad, ma, None, ts)
    with pytest.raises(ValueError, match="model 2.*sigsqr"):
        L.smooth_carma(t, y, e, np.r_[1.0, 1.0, 0.0], GOOD, ma, None, ts)
    with pytest.raises(ValueError, match="nma"):
        L.smooth_carma(t, y, e, sig, GOOD, np.ones((3, 4)), None, ts)
    with pytest.raises(ValueError, match="same number"):
        L.smooth_carma(t, y, e, np.ones(2), GOOD, ma, None, ts)
    with pytest.raises(ValueError, match="tout\\[2\\]"):
        L.smooth_carma(t, y, e, sig, GOOD, ma, None, np.r_[0.0, 1.0, np.nan])
    with pytest.raises(ValueError, match="M >= 1"):
        L.smooth_carma(t, y, e, sig, GOOD, ma, None, np.array([]))
    with pytest.raises(ValueError, match="band"):
        L.smooth_carma(t, y, e, sig, GOOD, ma, None, ts, band="both")
    with pytest.raises(ValueError, match="model 1.*omega"):
        L.smooth_car1(t, y, e, np.ones(3), np.r_[1.0, -1.0, 1.0], None, ts)
    with pytest.raises(ValueError, match="one entry per model"):
        L.smooth_car1(t, y, e, np.ones(3), np.ones(3), np.zeros(2), ts)
    # the raw entry point: K < 1, and outputs that do not come in pairs
    dp = C.POINTER(C.c_double)
    p_ = lambda a: a.ctypes.data_as(dp)                                      # noqa: E731
    om = np.ascontiguousarray(np.stack([GOOD.real, GOOD.imag], axis=-1))
    out = np.full((3, 7), 7.25)
    rc = L.lib.carma_smooth_carma(p_(t), p_(y), p_(e), t.size, 3, 0, p_(sig), p_(om), p_(ma), 1, None, p_(ts), 7, p_(out), p_(out),
                                  None, None, None, None, 0)
    assert rc == EINVAL and "nmodels >= 1" in L.last_error()
    rc = L.lib.carma_smooth_carma(p_(t), p_(y), p_(e), t.size, 3, 3, p_(sig), p_(om), p_(ma), 1, None, p_(ts), 7, p_(out), None,
                                  None, None, None, None, 0)
    assert rc == EINVAL and "pairs" in L.last_error()
    assert np.all(out == 7.25)


def test_the_chunk_switch_is_known():
    L = _lib()
    L.tune_set("SMOOTH_CHUNK_MODELS", 3)
    L.tune_set("SMOOTH_CHUNK_MODELS", None)
