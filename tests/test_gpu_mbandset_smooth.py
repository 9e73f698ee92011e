"""GPU tests of the smoother on a SET of multi-band objects (k_smooth_mband_fwd_ms / _bwd_ms behind carma_bandset_smooth,
BandsSetContext.smooth, CarmaBandsSet.smooth).  The yardstick is the single-object path (BandsContext.smooth,
CarmaBandsModel.smooth): a wave works on one job with the bodies of the single-object kernels, so every number is held to BIT
equality with it; tests/test_gpu_mband_smooth.py holds that path to the exact value, and the objects small enough for
mband_smooth_ref.dense_smooth_truth are held to it here as well (the project's smoother rule, 1e-9)."""
import ctypes as C
import functools

import numpy as np
import pytest

import mband_ref as R
import mband_smooth_ref as S
import test_gpu_mbandset as G

pytestmark = pytest.mark.gpu
CARMA_EINVAL = -22
ORDERS = [(1, 0), (2, 1), (5, 3), (7, 6)]
TIMES_M = [12, 1, 40, 25]


@pytest.fixture(scope="module")
def cpa():
    import carma_pack_amd
    assert carma_pack_amd._lib.lib.carma_device_count() >= 1
    return carma_pack_amd


@functools.lru_cache(None)
def times():
    """One list of observer times per object, M = 12, 1, 40 and 25: unsorted, the first before all data by more than any lag, the
    second behind them, the last a repeat of the third (M = 1: one time inside the data)."""
    rng = np.random.default_rng(77)
    out = []
    for o, M in zip(G.objects()[0], TIMES_M):
        lo, hi = min(b[0].min() for b in o), max(b[0].max() for b in o)
        t = rng.uniform(lo - 3.0, hi + 3.0, M)
        if M >= 3:
            t[0], t[1], t[-1] = lo - 30.0, hi + 30.0, t[2]
        out.append(t)
    return out


@functools.lru_cache(None)
def rows(p, q):
    """(thx [259, dx], which [259], band [259]): every row of test_gpu_mbandset.problem -- 63, 1, 65 and 130 of the four objects,
    shuffled, the ones outside the prior (which the smoother never applies) and the non-finite ones among them -- with an output
    band each."""
    thx, which = G.problem(p, q)
    band = np.random.default_rng(5 * p + q).integers(0, G.NBANDS, which.size)
    return thx, which, band


def _bits(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _same_rows(got, want):
    """got: (means, vars, invalid) of a set call; want: the same, row by row."""
    return len(got[0]) == len(want[0]) and _bits(got[0], want[0]) and _bits(got[1], want[1]) and np.array_equal(got[2], want[2])


@pytest.fixture(scope="module")
def single_rows(cpa):
    """{(p, q): (means, vars, invalid) of rows(p, q)} from BandsContext.smooth, one call per (object, band) group on a handle of
    the object alone: computed once per order."""
    cache = {}

    def get(p, q):
        if (p, q) not in cache:
            thx, which, band = rows(p, q)
            means, variances, inv = [None] * which.size, [None] * which.size, np.zeros(which.size, dtype=bool)
            for s in range(4):
                ctx = G.single(cpa, s, p, q)
                for b in range(G.NBANDS):
                    k = np.flatnonzero((which == s) & (band == b))
                    if k.size:
                        m, v, iv = ctx.smooth(thx[k], b, times()[s])
                        for j, i in enumerate(k):
                            means[i], variances[i], inv[i] = m[j], v[j], iv[j]
                ctx.close()
            cache[(p, q)] = (means, variances, inv)
        return cache[(p, q)]
    return get


def _set_call(st, thx, which, band):
    return st.smooth(thx, which, band, [times()[s] for s in which], return_invalid=True)


# ---- same bits as the single-object kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q", ORDERS)
def test_set_has_the_bits_of_the_single_object_kernels(cpa, single_rows, p, q):
    thx, which, band = rows(p, q)
    assert [int((which == s).sum()) for s in range(4)] == [63, 1, 65, 130] and [t.size for t in times()] == TIMES_M
    assert all(np.unique(t).size == t.size - 1 and np.any(np.diff(t) < 0) for t in times() if t.size > 1)
    assert set(band[which == 3]) == {0, 1, 2} and set(band[which == 0]) == {0, 1, 2}
    want = single_rows(p, q)
    assert 8 <= want[2].sum() < 40 and np.array_equal(want[2], np.isnan(thx).any(axis=1))
    assert all(np.all(np.isnan(m)) == bad and (bad or np.all(np.isfinite(m))) for m, bad in zip(want[0], want[2]))
    lib = cpa._lib
    st = G.make_set(cpa, p, q)
    got = _set_call(st, thx, which, band)
    assert all(m.shape == v.shape == times()[s].shape for m, v, s in zip(got[0], got[1], which))
    assert got[2].dtype == bool and _same_rows(got, want)
    for seed in (0, 1):
        perm = np.random.default_rng(seed).permutation(which.size)
        again = _set_call(st, thx[perm], which[perm], band[perm])
        assert _same_rows(again, ([want[0][i] for i in perm], [want[1][i] for i in perm], want[2][perm])), seed
    try:
        for waves in (1, 2):
            lib.tune_set("MBANDSET_SMOOTH_CHUNK_WAVES", waves)
            assert _same_rows(_set_call(st, thx, which, band), want), waves
    finally:
        lib.tune_set("MBANDSET_SMOOTH_CHUNK_WAVES", None)
    # one index for all rows, one array of times for all rows
    k = np.flatnonzero((which == 2) & (band == 1))
    one = st.smooth(thx[k], 2, 1, times()[2], return_invalid=True)
    assert _same_rows(one, ([want[0][i] for i in k], [want[1][i] for i in k], want[2][k]))
    st.close()


# ---- against the exact value ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q", ORDERS)
def test_small_objects_vs_dense_truth(cpa, p, q):
    objs, extras = G.objects()
    base = R.order_thetas(p, q)
    thx, which, bo, tl = [], [], [], []
    for s in (0, 1, 2):                                       # N = 6, 20, 40
        for i in range(2):                                    # rows 0 and 1 of the object in test_gpu_mbandset.problem: the plain ones
            x = R.extend(base[i], extras[s])                  # (object 1 has ONE row there; it gets the order's second vector too)
            if p == 1:
                t0 = objs[s][0][0]
                x[3] = 0.5 * (np.log(1.0 / np.diff(t0).min()) + np.log(1.0 / (t0.max() - t0.min())))
            assert np.sum(np.all(G.problem(p, q)[0] == x, axis=1) & (G.problem(p, q)[1] == s)) == (i < G.EVALS[s])
            for b in (0, G.NBANDS - 1):
                thx.append(x)
                which.append(s)
                bo.append(b)
                tl.append(times()[s][:6])
    st = G.make_set(cpa, p, q)
    means, variances = st.smooth(np.array(thx), which, bo, tl)
    st.close()
    for i, (x, s, b, t) in enumerate(zip(thx, which, bo, tl)):
        tm, tv = S.dense_smooth_truth(objs[s], x, p, q, b, t)
        em, ev = S.errors(means[i], variances[i], tm, tv)
        print("(%d,%d) object %d band %d row %d: device from the exact value: mean %.2e var %.2e" % (p, q, s, b, i, em, ev))
        assert np.all(np.isfinite(means[i])) and np.all(variances[i] > 0)
        assert em <= S.RTOL and ev <= S.RTOL


# ---- different times per row of one object -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q", [(2, 1), (7, 6)])
def test_rows_of_one_object_and_band_on_different_times(cpa, p, q):
    thx, which, _ = rows(p, q)
    k = np.flatnonzero((which == 2) & ~np.isnan(thx).any(axis=1))[:4]
    a, b = times()[2], times()[2][5:30][::-1].copy()
    tl = [a, b, a.copy(), b[:7]]                              # rows 0 and 2 on identical lists: one job; rows 1 and 3: a job each
    st = G.make_set(cpa, p, q)
    got = st.smooth(thx[k], 2, 1, tl, return_invalid=True)
    ctx = G.single(cpa, 2, p, q)
    for i in range(4):
        m, v, iv = ctx.smooth(thx[k[i]], 1, tl[i])
        assert np.array_equal(got[0][i], m) and np.array_equal(got[1][i], v) and got[2][i] == iv and not iv, i
    assert not np.array_equal(got[0][0], got[0][2])           # (other vectors: other curves)
    # the same vector twice on one list, once on a sub-list: a time's value does not depend on what else is asked for
    twice = st.smooth(thx[[k[0]] * 3], 2, 1, [a, a, a[:9]])
    assert _bits(twice[0][:2], [got[0][0]] * 2) and _bits(twice[1][:2], [got[1][0]] * 2)
    ctx.close()
    st.close()


# ---- an invalid row -----------------------------------------------------------------------------------------------------------------------
def test_invalid_row_is_nan_flagged_and_alone(cpa, single_rows):
    p, q = 5, 3
    thx, which, band = rows(p, q)
    want = single_rows(p, q)
    k = np.flatnonzero(~want[2])[:70]                         # valid rows of several objects and bands
    x = thx[k].copy()
    x[11, 3 + p + q] = np.nan                                 # the lag of band 1
    lib = cpa._lib
    st = G.make_set(cpa, p, q)
    got = _set_call(st, x, which[k], band[k])
    assert got[2].tolist() == [i == 11 for i in range(70)]
    assert np.all(np.isnan(got[0][11])) and np.all(np.isnan(got[1][11])) and got[0][11].shape == times()[which[k[11]]].shape
    keep = np.delete(np.arange(70), 11)
    assert _bits([got[0][i] for i in keep], [want[0][i] for i in k[keep]])
    assert _bits([got[1][i] for i in keep], [want[1][i] for i in k[keep]])
    with pytest.raises(lib.CarmaError, match=r"row\(s\) \[11\]"):
        st.smooth(x, which[k], band[k], [times()[s] for s in which[k]])
    # at the C level without the flag array: the call returns 1, and 0 without the row
    tl = [times()[s] for s in which[k]]
    toff = np.concatenate([[0], np.cumsum([t.size for t in tl])]).astype(np.int64)
    tp = np.concatenate(tl)
    w, bo = np.ascontiguousarray(which[k], dtype=np.int32), np.ascontiguousarray(band[k], dtype=np.int32)
    m, v = np.empty(tp.size), np.empty(tp.size)
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_long)
    rc = lib.lib.carma_bandset_smooth(st._h, lib.ptr(x), w.ctypes.data_as(ip), bo.ctypes.data_as(ip), 70, lib.ptr(tp),
                                      toff.ctypes.data_as(lp), lib.ptr(m), lib.ptr(v), None)
    assert rc == 1 and np.array_equal(m, np.concatenate(got[0]), equal_nan=True) and np.array_equal(v, np.concatenate(got[1]), equal_nan=True)
    rc = lib.lib.carma_bandset_smooth(st._h, lib.ptr(x), w.ctypes.data_as(ip), bo.ctypes.data_as(ip), 11, lib.ptr(tp),
                                      toff.ctypes.data_as(lp), lib.ptr(m), lib.ptr(v), None)
    assert rc == 0
    st.close()


# ---- argument errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors(cpa):
    lib = cpa._lib
    p, q = 2, 1
    thx, which, band = rows(p, q)
    k = np.flatnonzero(~np.isnan(thx).any(axis=1))[:3]
    x = np.ascontiguousarray(thx[k])
    w, bo = np.ascontiguousarray(which[k], dtype=np.int32), np.ascontiguousarray(band[k], dtype=np.int32)
    tp = np.array([-5.0, 4.0, -1.0, 11.5, 4.0, 2.0, 3.0, 3.0])
    toff = np.array([1, 4, 5, 8], dtype=np.int64)             # (the call's times start behind tp[0])
    st = G.make_set(cpa, p, q)
    before = st.smooth(x, w, bo, [tp[1:4], tp[4:5], tp[5:8]], return_invalid=True)
    m, v = np.full(7, -7.0), np.full(7, -7.0)
    inv = np.zeros(3, dtype=np.int32)
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_long)
    P, I, L = lib.ptr, (lambda a: a.ctypes.data_as(ip)), (lambda a: a.ctypes.data_as(lp))

    def arr(a, i, val):
        a = a.copy()
        a[i] = val
        return a

    def call(h=st._h, th=P(x), obj=I(w), b=I(bo), B=3, t=P(tp), off=L(toff), mean=P(m), var=P(v)):
        return lib.lib.carma_bandset_smooth(h, th, obj, b, B, t, off, mean, var, I(inv))

    keep = [arr(w, 1, 4), arr(w, 0, -1), arr(bo, 2, 3), arr(bo, 0, -1), arr(toff, 2, 4), arr(toff, 3, 4), arr(toff, 0, -1),
            arr(tp, 6, np.nan), arr(tp, 4, np.inf), arr(toff, 3, 2 ** 31)]
    cases = [(dict(h=None), "null handle"), (dict(B=0), "need B >= 1 (got B = 0)"), (dict(B=-2), "need B >= 1"),
             (dict(th=None), "non-null"), (dict(obj=None), "non-null"), (dict(b=None), "non-null"), (dict(t=None), "non-null"),
             (dict(off=None), "non-null"), (dict(mean=None), "non-null"), (dict(var=None), "non-null"),
             (dict(obj=I(keep[0])), "object[1] = 4 out of range (nobjects = 4)"), (dict(obj=I(keep[1])), "object[0] = -1 out of range"),
             (dict(b=I(keep[2])), "band[2] = 3 is outside [0, 3)"), (dict(b=I(keep[3])), "band[0] = -1 is outside [0, 3)"),
             (dict(off=L(keep[4])), "row 1 has no times"), (dict(off=L(keep[5])), "row 2 has no times"),
             (dict(off=L(keep[6])), "toff[0] = -1 is negative"), (dict(t=P(keep[7])), "time 1 of row 2 is not finite"),
             (dict(t=P(keep[8])), "time 0 of row 1 is not finite"),
             (dict(off=L(keep[9])), "row 2: more data and requested times than an int can count")]
    for kw, text in cases:
        assert call(**kw) == CARMA_EINVAL, kw
        msg = lib.last_error()
        assert msg.startswith("carma_bandset_smooth: ") and text in msg, (kw, msg)
    assert np.all(m == -7.0) and np.all(v == -7.0) and not inv.any()          # nothing was written
    assert call(t=P(arr(tp, 0, np.nan))) == 0                                  # in front of toff[0]: not the call's
    assert np.array_equal(m, np.concatenate(before[0])) and np.array_equal(v, np.concatenate(before[1]))
    with pytest.raises(ValueError, match=r"object\[0\] = 9"):
        st.smooth(x, 9, bo, tp)
    with pytest.raises(ValueError, match="one array per row"):
        st.smooth(x, w, bo, [tp, tp])
    assert _same_rows(st.smooth(x, w, bo, [tp[1:4], tp[4:5], tp[5:8]], return_invalid=True), before)   # the handle is as it was
    st.close()


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------
class _Fit(object):
    def __init__(self, x):
        self.x = x


def test_python_layer(cpa):
    from carma_pack_amd.carma_pack import CarmaBandsSet
    p, q = 2, 1
    objs = G.objects()[0]
    thx, which, _ = rows(p, q)
    ok = ~np.isnan(thx).any(axis=1)
    bs = CarmaBandsSet([objs[s] for s in (1, 2, 3)], p=p, q=q, lag_bounds=G.lag_boxes()[1:4])
    xs = [thx[ok & (which == s)][:3] for s in (1, 2, 3)]      # [1, dx] (object 1 has one row), [3, dx], [3, dx]
    assert [x.shape[0] for x in xs] == [1, 3, 3]
    one = times()[0]
    per = [times()[s] for s in (1, 2, 3)]

    def want(s, x, t, b):
        return bs.models[s].smooth(x, t, band=b)

    # vectors, one array of times, every band
    out = bs.smooth([x[0] for x in xs], one)
    assert len(out) == 3
    for s, (m, v) in enumerate(out):
        assert m.shape == v.shape == (3, one.size)
        for b in range(3):
            assert _bits((m[b], v[b]), want(s, xs[s][0], one, b))
    # arrays of rows, a list of S arrays of times, a list of bands
    out = bs.smooth(xs, per, band=[2, 0])
    for s, (m, v) in enumerate(out):
        assert m.shape == v.shape == (2, xs[s].shape[0], per[s].size)
        for j, b in enumerate((2, 0)):
            assert _bits((m[j], v[j]), want(s, xs[s], per[s], b))
    # what get_mle returns (objects with .x), an int band: neither a row axis nor a band axis
    out = bs.smooth([_Fit(x[-1]) for x in xs], per, band=1)
    for s, (m, v) in enumerate(out):
        assert m.shape == v.shape == (per[s].size,)
        assert _bits((m, v), want(s, xs[s][-1], per[s], 1))
    # mixed entries
    out = bs.smooth([xs[0][0], xs[1], _Fit(xs[2][1])], one, band=0)
    assert [o[0].shape for o in out] == [(one.size,), (3, one.size), (one.size,)]
    assert _bits(out[1], want(1, xs[1], one, 0)) and _bits(out[2], want(2, xs[2][1], one, 0))
    assert "smooth" in CarmaBandsSet.get_mle.__doc__
    bad = [x.copy() for x in xs]
    bad[1][2, 3 + p + q + 1] = np.nan                         # log a of band 1 of row 2 of object 1
    with pytest.raises(ValueError, match="object 1, row 2"):
        bs.smooth(bad, per)
    with pytest.raises(ValueError, match="one entry per object"):
        bs.smooth(xs[:2], per)
