"""CPU tests of the host-only planner of carma_bandset_smooth (carma_mband_set_smooth_plan.h as a stand-alone program,
tests/mbandset_smooth/plan_main.cpp): the jobs, waves, tables and chunks against a numpy restatement and against the properties
the kernels rely on, every argument refusal by its message, MbandSet::t0, and the same program under
-fsanitize=address,undefined."""
import numpy as np
import pytest

import mbandset_smooth_ref as P

CALLS = [(0, 300), (1, 300), (2, 129), (3, 64), (4, 65), (5, 1), (6, 7)]   # (seed, B)


def _same(got, want):
    for k, v in want.items():
        assert np.array_equal(got[k], v), k


def _properties(pl, p, nobj, t0, obj, band, times, forced, cap):
    B, W, J = len(obj), pl["W"], pl["J"]
    rows = pl["row_idx"]
    live = rows[rows >= 0]
    assert sorted(live.tolist()) == list(range(B))            # every row once
    assert np.all(rows[:, 0] >= 0)                            # lane 0 is live ...
    assert np.all(np.diff((rows >= 0).astype(int), axis=1) <= 0)   # ... and pads only trail
    assert W == rows.shape[0] and len(pl["wave_job"]) == W and J == len(pl["job_obj"])
    ng = np.asarray(nobj)[pl["job_obj"]] + pl["job_M"]
    assert np.all(np.diff(ng[pl["wave_job"]]) <= 0)           # the waves with the most points first
    seen = {}
    for w in range(W):
        j = pl["wave_job"][w]
        for i in rows[w][rows[w] >= 0]:                       # a wave holds ONE job: its rows share object, band and times
            assert obj[i] == pl["job_obj"][j] and band[i] == pl["job_band"][j] and len(times[i]) == pl["job_M"][j]
            assert np.array_equal(times[i], times[rows[w, 0]])
        key = (obj[rows[w, 0]], band[rows[w, 0]], tuple(times[rows[w, 0]]))
        assert seen.setdefault(key, j) == j                   # ... and equal keys are one job
        mine = rows[w][rows[w] >= 0]
        assert np.all(np.diff(mine) > 0)                      # the caller's order inside a wave
    assert len(seen) == J
    for j in range(J):                                        # only a job's LAST wave is padded
        ws = np.flatnonzero(pl["wave_job"] == j)
        assert np.all(rows[ws[:-1]] >= 0) and np.all(np.diff(ws) == 1)
        r0 = pl["job_req"][j]
        want = P.times_ref(times[rows[ws[0], 0]], t0[pl["job_obj"][j]])
        assert np.array_equal(pl["req"][r0:r0 + pl["job_M"][j] + 1], want)
    assert pl["req"].shape[0] == int(np.sum(pl["job_M"] + 1))
    assert np.array_equal(pl["out_off"], np.concatenate([[0], np.cumsum([len(t) for t in times])[:-1]]))
    # chunks: whole waves, one at least, inside the cap unless a wave alone exceeds it; a wave's records do not overlap another's
    c0 = pl["chunk0"]
    assert c0[0] == 0 and c0[-1] == W and np.all(np.diff(c0) >= 1)
    need = ng[pl["wave_job"]] * 64 * P.nfields(p)
    for a, b in zip(c0[:-1], c0[1:]):
        assert np.array_equal(pl["wave_sc"][a:b], np.concatenate([[0], np.cumsum(need[a:b])[:-1]]))
        assert 8 * need[a:b].sum() <= cap or b - a == 1
        assert forced <= 0 or b - a <= forced
        assert need[a:b].sum() <= pl["sc_max"]
        if b < W and (forced <= 0 or b - a < forced):         # cut by the cap: the next wave would not have fitted
            assert 8 * (need[a:b].sum() + need[b]) > cap
    assert pl["sc_max"] == max(need[a:b].sum() for a, b in zip(c0[:-1], c0[1:]))


@pytest.mark.parametrize("seed,B", CALLS)
def test_plan_vs_restatement_and_properties(seed, B):
    nobj, t0, obj, band, times = P.random_call(seed, B)
    assert {len(t) for t in times} <= set(range(1, 41))
    p = 1 + seed % 7
    got = P.plan(p, nobj, t0, obj, band, times, toff0=seed)
    _same(got, P.plan_ref(p, nobj, t0, obj, band, times))
    _properties(got, p, nobj, t0, obj, band, times, 0, P.CAP)
    assert len(got["chunk0"]) == 2                            # these calls fit the cap: one chunk
    if B == 300:
        assert got["J"] < got["W"] < B and np.any(np.bincount(got["wave_job"]) > 1)   # shared lists: jobs of several waves


@pytest.mark.parametrize("forced", [1, 2])
def test_forced_chunk_sizes(forced):
    nobj, t0, obj, band, times = P.random_call(0, 300)
    got = P.plan(5, nobj, t0, obj, band, times, forced=forced)
    _same(got, P.plan_ref(5, nobj, t0, obj, band, times, forced=forced))
    _properties(got, 5, nobj, t0, obj, band, times, forced, P.CAP)
    sizes = np.diff(got["chunk0"])
    assert np.all(sizes[:-1] == forced) and 1 <= sizes[-1] <= forced
    free = P.plan(5, nobj, t0, obj, band, times)
    for k in ("wave_job", "row_idx", "job_req", "out_off", "req"):   # the chunking moves nothing but the scratch
        assert np.array_equal(got[k], free[k])


def test_chunks_at_a_small_cap_and_below_one_wave():
    nobj, t0, obj, band, times = P.random_call(1, 300)
    p = 3
    need_max = (max(nobj) + 40) * 64 * P.nfields(p) * 8
    for cap in (3 * need_max, need_max // 50, 1):             # a few waves a chunk; some waves alone beyond it; every wave beyond it
        got = P.plan(p, nobj, t0, obj, band, times, cap=cap)
        _same(got, P.plan_ref(p, nobj, t0, obj, band, times, cap=cap))
        _properties(got, p, nobj, t0, obj, band, times, 0, cap)
    assert np.all(np.diff(got["chunk0"]) == 1)                # cap = 1: a wave a chunk all the same
    some = P.plan(p, nobj, t0, obj, band, times, cap=3 * need_max)
    assert 2 < len(some["chunk0"]) < some["W"]


def test_two_time_lists_on_one_object_and_band():
    nobj, t0 = [10, 20], [0.5, -2.0]
    a, b = np.array([3.0, 1.0, 3.0]), np.array([3.0, 1.0, 2.0])
    got = P.plan(2, nobj, t0, [1, 1, 1, 1, 0], [2, 2, 2, 2, 2], [a, b, a.copy(), b[:2], a])
    assert got["J"] == 4 and got["W"] == 4
    # the jobs in their sorted order: (0, a) (1, b[:2]) (1, b) (1, a), of ng = 13, 22, 23, 23; the waves by falling ng, ties as the jobs
    assert got["job_obj"].tolist() == [0, 1, 1, 1] and got["job_M"].tolist() == [3, 2, 3, 3]
    assert got["wave_job"].tolist() == [2, 3, 1, 0]
    assert got["row_idx"][:, :3].tolist() == [[1, -1, -1], [0, 2, -1], [3, -1, -1], [4, -1, -1]]
    _properties(got, 2, nobj, t0, [1, 1, 1, 1, 0], [2, 2, 2, 2, 2], [a, b, a, b[:2], a], 0, P.CAP)


def test_wave_order_is_by_points_first():
    got = P.plan(2, [10, 20], [0.0, 0.0], [0, 1, 0], [0, 0, 1], [np.arange(15.0), np.arange(3.0), np.arange(12.0)])
    ng = np.array([10, 20])[got["job_obj"]] + got["job_M"]
    assert ng[got["wave_job"]].tolist() == [25, 23, 22]


def test_argument_refusals():
    assert P.check() == ""
    assert P.check(h=0) == "null handle"
    assert P.check(obj=(), band=(), toff=(0,)) == "need B >= 1 (got B = 0)"
    for name in ("theta", "object", "band", "tout", "toff", "mean", "var"):
        assert P.check(null=(name,)) == "need non-null theta, object, band, tout, toff, mean and var", name
    assert P.check(obj=(0, 4)) == "object[1] = 4 out of range (nobjects = 4)"
    assert P.check(obj=(-1, 2)) == "object[0] = -1 out of range (nobjects = 4)"
    assert P.check(band=(0, 3)) == "band[1] = 3 is outside [0, 3)"
    assert P.check(band=(-2, 0)) == "band[0] = -2 is outside [0, 3)"
    assert P.check(toff=(5, 5, 9)) == "row 0 has no times: toff must grow by at least 1 a row (toff[0] = 5, toff[1] = 5)"
    assert P.check(toff=(5, 8, 7)) == "row 1 has no times: toff must grow by at least 1 a row (toff[1] = 8, toff[2] = 7)"
    assert P.check(toff=(-1, 2, 3)) == "toff[0] = -1 is negative"
    t = 0.5 * np.arange(9)
    t[7] = np.nan
    assert P.check(tout=t) == "time 2 of row 0 is not finite"
    t[7], t[8] = 1.0, np.inf
    assert P.check(tout=t) == "time 0 of row 1 is not finite"
    t[8], t[2] = 1.0, np.nan
    assert P.check(tout=t) == ""                              # in front of toff[0]: not the call's
    # N_s + M_i beyond an int: refused before a time is read
    assert P.check(nobj=(6, 20, 40, 2 ** 31 - 3), toff=(5, 8, 10)) == ""                     # 2^31 - 1 points: the last an int counts
    assert P.check(nobj=(6, 20, 40, 2 ** 31 - 3), toff=(5, 7, 10)) == "row 1: more data and requested times than an int can count"
    assert (P.check(toff=(0, 2 ** 31 - 6, 2 ** 31 - 5), tout=np.zeros(4))
            == "row 0: more data and requested times than an int can count")


def test_set_keeps_the_time_origin_of_every_object():
    rng = np.random.default_rng(7)
    objects = []
    for s in range(4):
        bands = []
        for b in range(3):
            n = int(rng.integers(1, 9)) + (1 if b == 0 else 0)
            t = np.round(rng.uniform(-30.0, 30.0) + rng.permutation(40)[:n] * 0.25, 2)     # unsorted, distinct
            bands.append((t, rng.standard_normal(n), rng.uniform(0.1, 0.2, n)))
        objects.append(bands)
    of_set, alone = P.set_t0(objects)
    want = [min(b[0].min() for b in o) for o in objects]
    assert np.array_equal(of_set, alone) and np.array_equal(of_set, want) and len(set(want)) == 4


def test_planner_under_address_and_undefined_behaviour_sanitizers():
    """The same stand-alone program built with -fsanitize=address,undefined and run directly: the plans and the checks of the
    tests above, with the same answers."""
    for seed, B in CALLS[:3]:
        nobj, t0, obj, band, times = P.random_call(seed, B)
        for forced, cap in ((0, 0), (1, 0), (0, 1), (2, 10 ** 6)):
            got = P.plan(4, nobj, t0, obj, band, times, toff0=3, forced=forced, cap=cap, sanitized=True)
            _same(got, P.plan_ref(4, nobj, t0, obj, band, times, forced=forced, cap=cap or P.CAP))
    assert P.check(sanitized=True) == ""
    assert P.check(obj=(0, 4), sanitized=True) == "object[1] = 4 out of range (nobjects = 4)"
    assert P.check(toff=(5, 8, 7), sanitized=True).startswith("row 1 has no times")
    assert P.check(tout=np.full(9, np.nan), sanitized=True) == "time 0 of row 0 is not finite"
    assert P.check(obj=(), band=(), toff=(0,), sanitized=True) == "need B >= 1 (got B = 0)"
