"""CPU-only: the host-only decisions of the calls on a set of multi-band objects (carma_pack_amd/csrc/carma_mband_set_plan.h through
tests/mbandset/mbandset_host.cpp) -- the create checks name the object, the lock-step optimiser keeps every point on its start's
object and fixed lags and the starts apart, the launch plan puts one object on a wave -- and the argument errors of
CarmaBandsSet that need no device."""
import numpy as np
import pytest

import mband_ref as R
import mbandset_build as MB


# ---- carma_bandset_create's checks ------------------------------------------------------------------------------------------
def _objects(S=3, K=2, n=(6, 4)):
    rng = np.random.default_rng(7)
    return [[R._band(rng, n[b], t0=float(b)) for b in range(K)] for _ in range(S)]


def _lags(S, K):
    return np.full((S, K - 1), -3.0), np.full((S, K - 1), 3.0)


def test_create_checks_pass_a_good_set():
    objs = _objects()
    t, y, e, off = MB.flat_set(objs)
    assert off.size == 3 * 2 + 1
    assert MB.check_create(t, y, e, off, 3, 2, 2, 1, *_lags(3, 2)) == ""
    one = [[b[0]] for b in objs]                              # one band: no lag boxes needed
    t1, y1, e1, off1 = MB.flat_set(one)
    assert MB.check_create(t1, y1, e1, off1, 3, 1, 2, 1, None, None) == ""


def test_create_checks_name_the_object():
    objs = _objects()
    t, y, e, off = MB.flat_set(objs)
    lo, hi = _lags(3, 2)
    # a wrong offset table: not from 0; a band boundary of object 1 that runs backwards
    bad = off.copy()
    bad[0] = 1
    assert MB.check_create(t, y, e, bad, 3, 2, 2, 1, lo, hi) == "offsets[0] must be 0"
    bad = off.copy()
    bad[3] = bad[2] - 1
    msg = MB.check_create(t, y, e, bad, 3, 2, 2, 1, lo, hi)
    assert msg.startswith("object 1: band 0 is empty or offsets decrease"), msg
    # an empty band: band 1 of object 2
    bad = off.copy()
    bad[6] = bad[5]
    msg = MB.check_create(t, y, e, bad, 3, 2, 2, 1, lo, hi)
    assert msg.startswith("object 2: band 1 is empty"), msg
    # a datum that is not finite: the third of object 1 (its own count)
    for arr in (0, 1, 2):
        cols = [t.copy(), y.copy(), e.copy()]
        cols[arr][off[2] + 2] = np.nan if arr else np.inf
        assert MB.check_create(cols[0], cols[1], cols[2], off, 3, 2, 2, 1, lo, hi) == "object 1: datum 2 is not finite"
    # an inverted lag box, a lag box that is not finite
    hi2 = hi.copy()
    hi2[2, 0] = -4.0
    msg = MB.check_create(t, y, e, off, 3, 2, 2, 1, lo, hi2)
    assert msg.startswith("object 2: lag box of band 1"), msg
    lo2 = lo.copy()
    lo2[0, 0] = -np.inf
    assert MB.check_create(t, y, e, off, 3, 2, 2, 1, lo2, hi).startswith("object 0: lag box of band 1")
    assert MB.check_create(t, y, e, off, 3, 2, 2, 1, None, hi).startswith("object 0: need lag_lo and lag_hi")
    # the set's own arguments
    assert "nobjects" in MB.check_create(t, y, e, off, 0, 2, 2, 1, lo, hi)
    assert "nbands" in MB.check_create(t, y, e, off, 3, 9, 2, 1, lo, hi)
    assert MB.check_create(t, y, e, off, 3, 2, 2, 2, lo, hi).startswith("object 0: need 1 <= p")


def test_one_datum_in_all_is_refused_per_object():
    rng = np.random.default_rng(1)
    objs = [[R._band(rng, 3)], [R._band(rng, 1)]]
    t, y, e, off = MB.flat_set(objs)
    assert MB.check_create(t, y, e, off, 2, 1, 1, 0, None, None) == "object 1: need at least 2 data in all"


# ---- the preparation: the set's slice of an object is the object's own preparation, byte for byte ---------------------------
def test_set_prepares_every_object_as_the_single_object_call_does():
    """S = 3 objects of K = 3 bands of 7, 1 and 12 data; one band is given unsorted, one has a repeated time.  The records from
    off[s], boff, n, N, lagbox and the three prior numbers of object s in the set equal, as bytes, what the object gives when it
    is prepared alone.  The set's C ABI takes max_stdev for every object or for none, so "one object given, the others on the
    default" is checked as both: every object once with max_stdev given and once on the default."""
    rng = np.random.default_rng(23)
    objs = [[R._band(rng, n, t0=0.25 * b + s) for b, n in enumerate((7, 1, 12))] for s in range(3)]
    t, y, e = objs[1][2]
    perm = rng.permutation(12)
    assert not np.all(np.diff(t[perm]) > 0)
    objs[1][2] = (t[perm], y[perm], e[perm])                  # object 1, band 2: unsorted
    t, y, e = (a.copy() for a in objs[2][0])
    t[4] = t[3]                                               # object 2, band 0: a repeated time (6 data are left of 7)
    objs[2][0] = (t, y, e)
    lo = np.array([[-1.0, -2.0], [-0.5, 0.0], [-3.0, 1.0]])
    hi = np.array([[1.0, 2.0], [0.5, 4.0], [3.0, 1.5]])
    for ms in (None, np.array([3.5, 0.75, 12.0])):
        got = [MB.prepared(objs, lo, hi, ms, s, alone=False) for s in range(3)]
        for s in range(3):
            assert got[s] == MB.prepared(objs, lo, hi, ms, s, alone=True), (s, ms)
        assert len(set(got)) == 3                             # ... and the objects differ
        # the layout of the bytes: 7 + 1 + 12 data (6 + 1 + 12 with the repeated time) and 3 sentinels, 4 doubles a record
        for s, ndata in enumerate((20, 20, 19)):
            assert len(got[s]) == 8 * 4 * (ndata + 3) + 4 * (4 + 3 + 1) + 8 * 4 + 8 * 3
            assert ms is None or np.frombuffer(got[s][-24:])[0] == ms[s]                 # max_stdev: the first prior number
    # the default of an object is 10 sqrt(var(y, ddof=1)) of its band 0 as given (to rounding: the loops' order is the library's)
    dflt = [np.frombuffer(MB.prepared(objs, lo, hi, None, s, alone=True)[-24:])[0] for s in range(3)]
    np.testing.assert_allclose(dflt, [10.0 * np.std(o[0][1], ddof=1) for o in objs], rtol=1e-13)


# ---- the boxes of carma_bandset_mle_batched -----------------------------------------------------------------------------------
def test_boxes_are_cut_to_the_lag_boxes_of_each_starts_object():
    d, K = 4, 3
    dx = d + 3 * (K - 1)
    lagbox = np.array([[[-1.0, 1.0], [-2.0, 2.0]], [[5.0, 6.0], [0.0, 0.5]]])           # [S][K - 1][2]
    which = np.array([1, 0, 1])
    lo, hi = np.full((3, dx), -np.inf), np.full((3, dx), np.inf)
    lo[1, d], hi[1, d + 3] = -0.25, 1.5
    lo[2, 0], hi[2, 0] = 0.1, 0.2
    lo2, hi2, bad, _ = MB.cut_boxes(lo, hi, which, d, K, lagbox)
    assert bad == -1
    for i in range(3):
        for b in (1, 2):
            c = d + 3 * (b - 1)
            assert lo2[i, c] == max(lo[i, c], lagbox[which[i], b - 1, 0]) and hi2[i, c] == min(hi[i, c], lagbox[which[i], b - 1, 1])
    rest = np.ones(dx, dtype=bool)
    rest[[d, d + 3]] = False
    assert np.array_equal(lo2[:, rest], lo[:, rest]) and np.array_equal(hi2[:, rest], hi[:, rest])
    # nothing left of band 2's box of start 2 (on object 1: [0, 0.5]); the same box is fine for start 1 (object 0)
    lo[2, d + 3] = lo[1, d + 3] = 0.75
    _, _, bad, band = MB.cut_boxes(lo, hi, which, d, K, lagbox)
    assert (bad, band) == (2, 2)
    assert MB.cut_boxes(lo, hi, which, d, K, lagbox, fixed=True)[2] == -1               # fixed lags: the entries are not read


# ---- mbandset_mle_run on a separable quadratic whose minimum depends on the object ------------------------------------------------
D, K3 = 4, 3
DX = D + 3 * (K3 - 1)
LAGC = [D, D + 3]
CENTRE = np.array([np.linspace(-1.0, 1.0, DX) * (s + 1) + 0.3 * s for s in range(3)])    # the minimum of object s
WEIGHT = np.linspace(0.5, 2.0, DX)
WHICH = np.array([0, 1, 2, 2, 1, 0, 1])


def _quad(skip):
    w = WEIGHT.copy()
    w[skip] = 0.0                                             # the columns that identify a start do not enter the objective

    def fun(pts, ob):
        return -np.sum(w * (pts - CENTRE[ob]) ** 2, axis=1)
    return fun


def _starts(seed=0):
    return np.random.default_rng(seed).uniform(-2.0, 2.0, (WHICH.size, DX))


def _free_problem():
    """Start i lives in [10 i, 10 i + 1] of column 0, which the objective ignores: a point names its start."""
    B = WHICH.size
    x0 = _starts()
    x0[:, 0] = 10.0 * np.arange(B) + 0.5
    lo, hi = np.full((B, DX), -np.inf), np.full((B, DX), np.inf)
    lo[:, 0], hi[:, 0] = 10.0 * np.arange(B), 10.0 * np.arange(B) + 1.0
    return x0, lo, hi


def test_mle_free_every_point_is_on_its_starts_object_and_every_start_reaches_its_minimum():
    x0, lo, hi = _free_problem()
    x, f, nit, status, calls = MB.mle(_quad([0]), D, K3, x0, WHICH, lo, hi)
    assert len(calls) > 3
    for pts, ob in calls:
        start = np.floor(pts[:, 0] / 10.0).astype(int)
        assert np.all((pts[:, 0] >= lo[start, 0]) & (pts[:, 0] <= hi[start, 0]))
        assert np.array_equal(ob, WHICH[start])
    assert np.all(status < 2) and np.all(nit > 0)
    np.testing.assert_allclose(x[:, 1:], CENTRE[WHICH][:, 1:], atol=1e-4)
    assert np.all(f < 1e-8)
    # one call per optimiser step carries the points of several objects
    assert sum(np.unique(ob).size == 3 for _, ob in calls) >= 3


def test_mle_fixed_lags_ride_with_their_start():
    B = WHICH.size
    x0 = _starts(1)
    fixed = np.stack([0.125 * np.arange(B) + 3.0, -0.25 * np.arange(B) - 1.0], axis=1)   # unique per start, exact in binary
    lo, hi = np.full((B, DX), -np.inf), np.full((B, DX), np.inf)
    lo[:, LAGC], hi[:, LAGC] = 50.0, -50.0                                               # not read with fixed lags
    x0[:, LAGC] = np.nan                                                                 # ... nor these
    x, f, nit, status, calls = MB.mle(_quad(LAGC), D, K3, x0, WHICH, lo, hi, fixed_lag=fixed)
    for pts, ob in calls:
        start = np.rint((pts[:, D] - 3.0) / 0.125).astype(int)
        assert np.array_equal(pts[:, LAGC], fixed[start])                                # both lags, exactly those of one start
        assert np.array_equal(ob, WHICH[start])
    assert np.array_equal(x[:, LAGC], fixed)
    rest = [j for j in range(DX) if j not in LAGC]
    assert np.all(status < 2)
    np.testing.assert_allclose(x[:, rest], CENTRE[WHICH][:, rest], atol=1e-4)


@pytest.mark.parametrize("fixed", [False, True])
def test_mle_starts_do_not_influence_each_other(fixed):
    B = WHICH.size
    if fixed:
        x0, lo, hi = _starts(2), np.full((B, DX), -3.0), np.full((B, DX), 3.0)
        fl = np.stack([0.125 * np.arange(B), -0.25 * np.arange(B)], axis=1)
        fun = _quad(LAGC)
    else:
        (x0, lo, hi), fl, fun = _free_problem(), None, _quad([0])
    lo[3, 2], hi[3, 2] = CENTRE[WHICH[3], 2] + 0.5, CENTRE[WHICH[3], 2] + 0.75           # one start ends on a bound of its own box
    ref = MB.mle(fun, D, K3, x0, WHICH, lo, hi, fixed_lag=fl)[:4]
    assert ref[0][3, 2] == lo[3, 2]
    perm = np.array([4, 0, 6, 2, 5, 1, 3])
    got = MB.mle(fun, D, K3, x0[perm], WHICH[perm], lo[perm], hi[perm], fixed_lag=None if fl is None else fl[perm])[:4]
    for a, b in zip(ref, got):
        assert np.array_equal(a[perm], b)                     # the same bits
    # ... and a start alone gives what it gives in company
    alone = MB.mle(fun, D, K3, x0[2:3], WHICH[2:3], lo[2:3], hi[2:3], fixed_lag=None if fl is None else fl[2:3])
    assert np.array_equal(alone[0][0], ref[0][2]) and alone[1][0] == ref[1][2] and alone[2][0] == ref[2][2]


# ---- the launch plan ------------------------------------------------------------------------------------------------------------
def test_plan_a_wave_holds_one_object_pads_trail_longest_first():
    N = np.array([5, 40, 40, 3, 100, 7])
    counts = [1, 64, 65, 130, 0, 63]                          # object 4, the longest, has no evaluation in this call
    which = np.random.default_rng(3).permutation(np.repeat(np.arange(6), counts))
    wobj, eidx = MB.plan(which, N)
    assert wobj.size == sum((c + 63) // 64 for c in counts) == 1 + 1 + 2 + 3 + 0 + 1
    live = eidx >= 0
    assert np.all(live[:, 0])                                 # lane 0 is live
    assert np.all(live[:, :-1] | ~live[:, 1:])                # pads only trail
    assert np.array_equal(np.sort(eidx[live]), np.arange(which.size))                    # every evaluation once
    for w in range(wobj.size):
        assert np.all(which[eidx[w][live[w]]] == wobj[w])     # one object per wave
    # the longest object first, ties in object order: 1, 2 (40 each), then 5 (7), 0 (5), 3 (3)
    assert wobj.tolist() == [1, 2, 2, 5, 0, 3, 3, 3]
    # an object's evaluations in the caller's order, only its last wave padded
    for s in range(6):
        ws = np.flatnonzero(wobj == s)
        e = eidx[ws].ravel()
        assert np.array_equal(e[e >= 0], np.flatnonzero(which == s))
        assert np.all(live[ws[:-1]]) if ws.size else True
    assert live[wobj == 0].sum() == 1                         # one evaluation: 63 pad lanes


def test_plan_refuses_an_object_out_of_range_and_plans_nothing_for_no_evaluations():
    with pytest.raises(ValueError, match=r"object\[2\]"):
        MB.plan(np.array([0, 1, 3, 7]), np.array([4, 4, 4]))
    with pytest.raises(ValueError, match=r"object\[0\]"):
        MB.plan(np.array([-1]), np.array([4, 4, 4]))
    wobj, eidx = MB.plan(np.zeros(0, dtype=np.int32), np.array([4, 4]))
    assert wobj.size == 0 and eidx.shape == (0, 64)


# ---- CarmaBandsSet: argument errors raised without a device ----------------------------------------------------------------------
def _set_objects():
    rng = np.random.default_rng(11)
    return [[R._band(rng, 8), R._band(rng, 6, t0=1.0)] for _ in range(3)]


def test_bands_set_argument_errors_need_no_device():
    from carma_pack_amd import CarmaBandsSet
    import carmcmc
    assert carmcmc.CarmaBandsSet is CarmaBandsSet
    objs = _set_objects()
    with pytest.raises(ValueError, match="at least one object"):
        CarmaBandsSet([])
    with pytest.raises(ValueError, match="object 1 has 1 bands, object 0 has 2"):
        CarmaBandsSet([objs[0], objs[1][:1], objs[2]], p=2, q=1)
    with pytest.raises(ValueError, match="object 2: band 1"):
        CarmaBandsSet([objs[0], objs[1], [objs[2][0], objs[2][1][:2]]], p=2, q=1)
    with pytest.raises(ValueError, match="lag_bounds"):
        CarmaBandsSet(objs, p=2, q=1, lag_bounds=[(-1.0, 1.0), (-2.0, 2.0)])
    bs = CarmaBandsSet(objs, p=2, q=1, lag_bounds=[(-1.0, 1.0), (-2.0, 2.0), (-3.0, 3.0)])       # one list per object
    assert [m.lag_bounds.tolist() for m in bs.models] == [[[-1.0, 1.0]], [[-2.0, 2.0]], [[-3.0, 3.0]]]
    assert (bs.nobjects, bs.K, bs.dx) == (3, 2, 3 + 2 + 1 + 3)
    with pytest.raises(ValueError, match=r"starts must be \[3, ntrials, 9\]"):
        bs.get_mle(starts=np.zeros((3, 4, 8)))
    with pytest.raises(ValueError, match=r"starts must be \[3, ntrials, 9\]"):
        bs.get_mle(starts=np.zeros((2, 4, 9)))
    with pytest.raises(ValueError, match="starts must be None, 'set'"):
        bs.get_mle(starts="all")
    with pytest.raises(ValueError, match="object 0: every lag must lie inside its box"):
        bs.lag_profile([0.0, 1.5])                            # inside the boxes of objects 1 and 2 only
    with pytest.raises(ValueError, match="object 1: every lag must lie inside its box"):
        bs.lag_profile([[0.0, 1.0], [0.0, 2.5], [0.0, 2.5]])  # one grid per object
    with pytest.raises(ValueError, match=r"lags must be \[L\]"):
        bs.lag_profile(np.zeros((4, 2)))
    with pytest.raises(ValueError, match="object index out of range"):
        bs.loglik(np.zeros(9), 3)
    allb = CarmaBandsSet(objs, p=1, lag_bounds=[(-5.0, 5.0)])                             # one list for all objects
    assert all(m.lag_bounds.tolist() == [[-5.0, 5.0]] for m in allb.models)
    with pytest.raises(ValueError, match="at least two bands"):
        CarmaBandsSet([[o[0]] for o in objs], p=1).lag_profile([0.0])
