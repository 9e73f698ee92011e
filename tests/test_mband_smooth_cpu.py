"""CPU tests of the multi-band smoother: the device header compiled for the host (carma_mband_smooth.h through
tests/emu/emu_mband_smooth.cpp) and the numpy yardstick against the exact 50-digit values on the whole case table, and the
host-only planner (carma_mband_smooth_plan.h as a stand-alone program).  The bound is the project's smoother rule: 1e-9 for every
entry, means relative to max(|mean|, sd), variances relative to the exact variance."""
import numpy as np
import pytest

import mband_ref as R
import mband_smooth_build as B
import mband_smooth_ref as S


# ---- the header and the yardstick against the exact value -------------------------------------------------------------------------
@pytest.mark.parametrize("p,q,name", R.CASES)
def test_header_vs_dense_truth(p, q, name):
    bands, thx, table = S.smooth_case(p, q, name)
    assert sorted(table) == S.table_bands(len(bands)) and thx.shape[0] == 2
    for bo, (tout, tm, tv) in table.items():
        assert tout.size == 12 and np.unique(tout).size == 11 and np.any(np.diff(tout) < 0)      # one repeat, unsorted
        mean, var, inv = B.smooth(bands, p, q, thx, bo, tout)
        em, ev = S.errors(mean, var, tm, tv)
        print("%s (%d,%d) band %d: header from the exact value: mean %.2e var %.2e" % (name, p, q, bo, em, ev))
        assert not inv.any() and np.all(np.isfinite(mean)) and np.all(var > 0)
        assert em <= S.RTOL and ev <= S.RTOL
        i, j = np.flatnonzero(tout == tout[np.argmax([np.sum(tout == v) for v in tout])])
        assert np.array_equal(mean[:, i], mean[:, j]) and np.array_equal(var[:, i], var[:, j])   # the repeated time: equal bits


@pytest.mark.parametrize("p,q,name", R.CASES)
def test_numpy_reference_vs_dense_truth(p, q, name):
    bands, thx, table = S.smooth_case(p, q, name)
    for bo, (tout, tm, tv) in table.items():
        mean, var = S.kalman_smooth_ref(bands, thx, p, q, bo, tout)
        em, ev = S.errors(mean, var, tm, tv)
        print("%s (%d,%d) band %d: kalman_smooth_ref from the exact value: mean %.2e var %.2e" % (name, p, q, bo, em, ev))
        assert em <= S.RTOL and ev <= S.RTOL
        one = S.kalman_smooth_ref(bands, thx[1], p, q, bo, tout)
        assert one[0].shape == (12,) and np.array_equal(one[0], mean[1]) and np.array_equal(one[1], var[1])


def test_tie_sits_on_a_datum_where_the_grid_is_exact():
    """The requested time meant as a tie is bit-equal to a shifted datum time of another band in the scenarios on the 1/4 grid."""
    for name in ("lag_equals_offset", "three_bands_7_1_12", "lag0_shared_stamps"):
        bands, thx, table = S.smooth_case(2, 1, name)
        lag, _, _ = R._band_params(thx[0], 6, len(bands))
        for bo, (tout, _, _) in table.items():
            others = np.concatenate([np.asarray(t) - lag[b] for b, (t, _, _) in enumerate(bands) if b != bo])
            assert np.intersect1d(tout - lag[bo], others).size >= 1, (name, bo)


def test_invalid_rows_are_flagged_and_walked():
    bands, thx, table = S.smooth_case(4, 2, "three_bands_7_1_12")
    tout = table[0][0]
    d = 9
    rows = np.tile(thx[0], (5, 1))
    rows[1, d] = np.nan                                       # lag of band 1
    rows[2, d + 4] = np.inf                                   # log a of band 2
    rows[3, d + 5] = -np.inf                                  # mu of band 2
    rows[4, 5:7] = rows[4, 3:5]                               # two equal quadratic factors: a repeated AR root
    mean, var, inv = B.smooth(bands, 4, 2, rows, 0, tout)
    assert list(inv) == [0, 1, 1, 1, 1]
    assert np.all(np.isnan(mean[1:])) and np.all(np.isnan(var[1:]))
    assert np.array_equal(mean[0], B.smooth(bands, 4, 2, thx[0], 0, tout)[0][0])


# ---- the planner ----------------------------------------------------------------------------------------------------------------------
def test_plan_times_permutation_is_stable():
    tout = np.array([5.0, -1.0, 3.0, 5.0, 3.0, 3.0, 100.25, -1.0])
    perm, rec = B.plan_times(tout, 2.5)
    assert list(perm) == list(np.argsort(tout, kind="stable")) == [1, 7, 2, 4, 5, 0, 3, 6]
    assert rec.shape == (9, 4)
    assert np.array_equal(rec[:8, 0], tout[perm] - 2.5) and np.array_equal(rec[:8, 1], perm.astype(float))
    assert np.all(rec[:8, 2:] == 0.0)
    assert np.isposinf(rec[8, 0]) and list(rec[8, 1:]) == [0.0, 1.0, 0.0]
    perm1, rec1 = B.plan_times([7.0], 0.0)
    assert list(perm1) == [0] and rec1.shape == (2, 4) and rec1[0, 0] == 7.0


@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 6, 7])
def test_plan_strides(p):
    ng = 37
    s = B.plan_strides(p, ng)
    fields = 2 * p + p // 2 + 5                               # k, cr, sr of every pair, {pm, f, s, innov | slot, a}
    assert s == dict(fields=fields, fs=64, ps=64 * fields, ws=64 * fields * ng)


def test_plan_chunks():
    p, ng = 5, 640
    row = 8 * (2 * p + p // 2 + 5) * ng                       # bytes of a row
    cap = 256 << 20
    waves = cap // (64 * row)
    assert waves >= 2
    auto = B.plan_chunks(p, ng, 10 ** 6, 0)
    assert auto == dict(rows=64 * waves, waves=waves, chunks=-(-10 ** 6 // (64 * waves)), bytes=waves * 64 * row)
    assert auto["bytes"] <= cap < auto["bytes"] + 64 * row    # at the cap: one more wave would not fit
    assert B.plan_chunks(p, ng, 10 ** 6, -5) == auto
    small = B.plan_chunks(p, ng, 130, 0)                      # fewer rows than the cap holds: one chunk of them
    assert small == dict(rows=130, waves=3, chunks=1, bytes=3 * 64 * row)
    forced = B.plan_chunks(p, ng, 130, 64)
    assert forced == dict(rows=64, waves=1, chunks=3, bytes=64 * row)
    one = B.plan_chunks(p, ng, 130, 1)
    assert one == dict(rows=1, waves=1, chunks=130, bytes=64 * row)
    assert B.plan_chunks(p, ng, 1, 0) == dict(rows=1, waves=1, chunks=1, bytes=64 * row)
    assert B.plan_chunks(p, ng, 5, 1000)["rows"] == 5        # never more rows than the call holds
    tiny = B.plan_chunks(p, ng, 1000, 0, cap=1)               # a cap below one wave: one wave all the same
    assert tiny == dict(rows=64, waves=1, chunks=16, bytes=64 * row)


def test_plan_argument_errors():
    assert B.plan_check() == ""
    assert B.plan_check(mean=0, var=0, bmean=1, bvar=1) == ""
    assert B.plan_check(h=0) == "null handle"
    assert B.plan_check(B=0) == "need B >= 1 and M >= 1 (got B = 0, M = 3)"
    assert B.plan_check(M=0) == "need B >= 1 and M >= 1 (got B = 1, M = 0)"
    assert B.plan_check(theta=0) == "need non-null theta and tout"
    assert B.plan_check(tout=0) == "need non-null theta and tout"
    assert B.plan_check(band=-1) == "band -1 is outside [0, 2)"
    assert B.plan_check(band=2) == "band 2 is outside [0, 2)"
    pairs = "mean and var, band_mean and band_var come in pairs, and one pair at least is needed"
    assert B.plan_check(var=0) == pairs
    assert B.plan_check(bmean=1) == pairs
    assert B.plan_check(mean=0, var=0) == pairs
    assert B.plan_check(bad=2) == "tout[2] is not finite"
    assert B.plan_check(bad=-2) == "tout[0] is not finite"
    assert B.plan_check(N=2 ** 31 - 3, M=3) == "more data and requested times than an int can count"
