"""CPU-only: the host-only launch planners of the multi-series calls (carma_pack_amd/csrc/carma_mseries_plan.h: the counting sort
by series, check_toff and the plans of carma_mlogdensity_batch, carma_mkfilter, carma_mpredict and carma_msmooth) through the
stand-alone program tests/mseries/plan_main.cpp, built and run here WITHOUT sanitizers.  Every table must equal the numpy
restatement tests/mseries_plan_ref.py exactly, and must have the properties the kernels rely on, asserted here on the program's
output alone."""
import functools
import os
import subprocess

import numpy as np
import pytest

import mseries_plan_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "carma_pack_amd", "csrc")
PLAN_H = os.path.join(CSRC, "carma_mseries_plan.h")
MAIN_SRC = os.path.join(HERE, "mseries", "plan_main.cpp")
MAIN_EXE = os.path.join(HERE, "mseries", "plan_main")
DEPS = [MAIN_SRC, PLAN_H, os.path.join(CSRC, "carma_smooth_plan.h")]


@functools.lru_cache(None)
def build_main():
    if not os.path.exists(MAIN_EXE) or any(os.path.getmtime(d) > os.path.getmtime(MAIN_EXE) for d in DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", MAIN_EXE, MAIN_SRC], check=True, timeout=300)
    return MAIN_EXE


def run(mode, *arrays):
    """the case as one line of numbers per array (floats with 17 digits) -> {name: int64 array, or float64 for `grids`}"""
    text = "\n".join(" ".join(repr(float(v)) if isinstance(v, (float, np.floating)) else str(int(v)) for v in np.atleast_1d(a))
                     for a in arrays)
    r = subprocess.run([build_main(), mode], input=text + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        name, *vals = line.split()
        out[name] = np.array(vals, dtype=np.float64 if name == "grids" else np.int64)
    return out


def same(got, want):
    """every table of the reference, exactly"""
    assert set(got) == set(want)
    for name, w in want.items():
        w = np.atleast_1d(np.asarray(w))
        assert got[name].shape == w.shape and np.array_equal(got[name], w), name


def test_the_header_needs_no_hip():
    """carma_mseries_plan.h includes the standard library and carma_smooth_plan.h only: a plain C++ compiler takes it on its own"""
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-x", "c++", PLAN_H], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    text = open(PLAN_H).read()
    assert "#include <hip" not in text and "set_error" not in text


# ---- check_toff -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("toff, want", [([0, 2, 2, 5], -1), ([3, 3, 4, 9], -1), ([-1, 2, 3, 5], -2), ([4, 3, 5, 6], 0), ([0, 2, 5, 4], 2),
                                        ([0, 5, 4, 3], 1)])
def test_check_toff(toff, want):
    """negative toff[0]; a decrease at item 0, at item M - 1, and the FIRST of two; toff[0] > 0 and an item without times are fine"""
    got = run("toff", [len(toff) - 1], toff)
    assert int(got["toff"][0]) == want == ref.check_toff(toff)


# ---- the sampler's chunk (carma_mpt_*) -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nmax, want", [(1, 4096), (1000, int(250000.0 / 450.0)), (10 ** 6, 1)])
def test_mpt_chunk_iters(nmax, want):
    """min(4096, 250000 / max(1, 0.45 nmax)), at least 1: the upper clamp, a value between (555), the lower clamp"""
    assert int(run("chunk", [nmax])["chunk"][0]) == want == max(1, int(min(4096.0, 250000.0 / max(1.0, 0.45 * nmax))))


# ---- log-density plan -----------------------------------------------------------------------------------------------------
# S = 5 series; series 2 never has evaluations; both cadence classes; series 0 and 4 tie in length within the plain class
LD_NSER = np.array([120, 300, 77, 45, 120])
LD_REPDT = np.array([0, 1, 0, 1, 0])


def _ld_series(B):
    rng = np.random.default_rng(100 + B)
    if B < 130:
        return rng.choice([0, 1, 3, 4], size=B, p=[0.4, 0.3, 0.2, 0.1])
    # series 4: exactly one full wave, no pad lane; series 1: a full wave and one lane more; series 0: a single lane
    return rng.permutation(np.repeat([4, 1, 0], [64, 65, 1]))


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_logdens_plan(B):
    series = _ld_series(B)
    got = run("logdens", [5, B], LD_NSER, LD_REPDT, series)
    same(got, ref.logdens(series, LD_NSER, LD_REPDT))
    W, w_plain = int(got["W"][0]), int(got["w_plain"][0])
    cnt = np.bincount(series, minlength=5)
    assert W == int(np.sum(-(-cnt // 64))) and got["wave_series"].size == W and got["eval_idx"].size == 64 * W
    ev = got["eval_idx"].reshape(W, 64)
    assert np.array_equal(np.sort(ev[ev >= 0]), np.arange(B))                    # every evaluation exactly once
    for w in range(W):
        live = ev[w] >= 0
        assert live[0] and not np.any(live[1:] & ~live[:-1])                     # lane 0 is live, pads only trail
        assert np.all(series[ev[w][live]] == got["wave_series"][w])              # a wave's lanes belong to its series
    ws = got["wave_series"]
    assert np.all(LD_REPDT[ws[:w_plain]] == 0) and np.all(LD_REPDT[ws[w_plain:]] == 1)
    for cls in (ws[:w_plain], ws[w_plain:]):
        assert np.all(np.diff(LD_NSER[cls]) <= 0)                                # longest first within a class
    assert 2 not in ws


@pytest.mark.parametrize("pos, bad", [(0, 5), (37, -1), (99, 7)])
def test_logdens_plan_names_the_first_bad_index(pos, bad):
    series = _ld_series(100)
    series[pos] = bad
    series[99] = 7 if pos != 99 else bad                      # a later one too: the FIRST is reported
    got = run("logdens", [5, 100], LD_NSER, LD_REPDT, series)
    assert set(got) == {"bad"} and int(got["bad"][0]) == pos == ref.logdens(series, LD_NSER, LD_REPDT)["bad"]


# ---- filter plan ----------------------------------------------------------------------------------------------------------
FI_NSER = np.array([2, 270, 31, 64, 150, 31, 9])              # series of 2 ... 270 points, two of equal length


@pytest.mark.parametrize("M", [1, 63, 64, 65, 130])
def test_filter_plan(M):
    series = np.random.default_rng(200 + M).integers(0, FI_NSER.size, M)
    got = run("filter", [FI_NSER.size, M], FI_NSER, series)
    same(got, ref.mfilter(series, FI_NSER))
    W = int(got["W"][0])
    order, n_item = got["order"], FI_NSER[series]
    slot_series, slot_n = got["tint"][:M], got["tint"][M:]
    tile_off, slot_out = got["tlong"][:W], got["tlong"][W:]
    assert W == -(-M // 64) and np.array_equal(np.sort(order), np.arange(M))     # a permutation ...
    assert np.all(np.diff(n_item[order]) <= 0)                                    # ... by length descending ...
    assert all(order[j] < order[j + 1] for j in range(M - 1) if n_item[order[j]] == n_item[order[j + 1]])   # ... and stable
    assert np.array_equal(slot_series, series[order]) and np.array_equal(slot_n, n_item[order])
    tiles = [2 * int(slot_n[64 * w]) * min(64, M - 64 * w) for w in range(W)]
    assert np.array_equal(tile_off, np.cumsum([0] + tiles)[:-1]) and int(got["tile_total"][0]) == sum(tiles)
    offs = np.concatenate([[0], np.cumsum(n_item)])
    assert np.array_equal(got["offs"], offs) and np.array_equal(slot_out, offs[order])   # the caller-order offset of the slot's item
    assert int(got["nmax"][0]) == n_item.max()


# ---- predict plan ---------------------------------------------------------------------------------------------------------
PR_NSER = np.array([40, 200, 90, 200])                        # series 1 and 3 tie in length; series 2 gets no item


@pytest.mark.parametrize("G", [0, 2, 4, 8])
def test_predict_plan(G):
    E = 64 // G if G else 64
    # the edges of test_gpu_mkalman.py: items with 0, 1, E - 1, E, E + 1 and 3 E + 1 times on one series, two more series
    counts = [0, 1, E - 1, E, E + 1, 3 * E + 1, E + 1, 2, 0, 5]
    series = np.array([1, 1, 1, 1, 1, 1, 0, 3, 3, 1])
    toff = 7 + np.concatenate([[0], np.cumsum(counts)])       # toff[0] > 0
    M, T = len(counts), int(sum(counts))
    got = run("predict", [G, PR_NSER.size, M], PR_NSER, series, toff)
    same(got, ref.predict(G, series, PR_NSER, toff))
    W = int(got["W"][0])
    assert int(got["T"][0]) == T and int(got["E"][0]) == E
    item_of = np.repeat(np.arange(M), counts)                 # output index -> item
    if not G:
        assert W == -(-T // 64) and np.array_equal(got["tint"][:M], series) and np.array_equal(got["tint"][M:], item_of)
        assert got["tlong"].size == 0
        return
    wave_series, pair_item, pair_out = got["tint"][:W], got["tint"][W:].reshape(W, E), got["tlong"].reshape(W, E)
    live = pair_out >= 0
    assert np.array_equal(np.sort(pair_out[live]), np.arange(T))                 # every output exactly once
    assert np.all(pair_out[~live] == -1) and np.all(live[:, 0])                  # idle groups carry -1; group 0 is live
    assert np.array_equal(pair_item[live], item_of[pair_out[live]])
    for w in range(W):
        assert np.all(series[pair_item[w][live[w]]] == wave_series[w])           # a wave's pairs lie on its series
    assert np.all(np.diff(PR_NSER[wave_series]) <= 0) and 2 not in wave_series   # longest series first
    npair = np.bincount(series, weights=counts, minlength=PR_NSER.size).astype(int)
    assert W == int(np.sum(-(-npair // E)))


# ---- smooth plan ----------------------------------------------------------------------------------------------------------
SM_NSER = np.array([12, 30, 7])


def _smooth_case(G):
    """items that share (series, times) in groups of 1, E and E + 1, an item without times, two items whose times differ in the
    last value only -- shuffled, with unused times in front (toff[0] > 0)"""
    E = 64 // G if G else 64
    rng = np.random.default_rng(300 + G)
    t_all = np.concatenate([np.cumsum(rng.uniform(0.5, 2.0, n)) for n in SM_NSER])
    lists = {"a": (1, rng.uniform(0, 20, 5)), "b": (0, rng.uniform(0, 20, 3)), "c": (1, rng.uniform(0, 20, 4))}
    near = lists["b"][1].copy()
    near[-1] += 1e-9
    items = [("a", 1), ("b", E), ("c", E + 1)]
    spec = [(lists[k][0], lists[k][1]) for k, m in items for _ in range(m)]
    spec += [(2, np.zeros(0)), (0, near), (2, np.array([3.0, 3.0, -4.0]))]
    spec = [spec[i] for i in rng.permutation(len(spec))]
    series = np.array([s for s, _ in spec])
    toff = 4 + np.concatenate([[0], np.cumsum([x.size for _, x in spec])])
    tout = np.concatenate([rng.uniform(0, 1, 4)] + [x for _, x in spec])
    return E, series, t_all, toff, tout


@pytest.mark.parametrize("forced", [0, "E"])
@pytest.mark.parametrize("G", [0, 2, 4, 8])
def test_smooth_plan(G, forced):
    E, series, t_all, toff, tout = _smooth_case(G)
    forced = E if forced == "E" else 0
    M, T = series.size, int(toff[-1] - toff[0])
    got = run("smooth", [G, SM_NSER.size, M, forced], SM_NSER, t_all, series, toff, tout)
    same(got, ref.smooth(G, series, SM_NSER, t_all, toff, tout, forced))
    W, J = int(got["W"][0]), int(got["J"][0])
    assert int(got["E"][0]) == E
    # jobs: a (1 item), b (E), b with another last value (1), c (E + 1), the three times on series 2 (1)
    assert J == 5 and W == 1 + 1 + 1 + 2 + 1
    ti, tl = got["tint"], got["tlong"]
    wave_job, job_series, job_ng = ti[:W], ti[W:W + J], ti[W + J:W + 2 * J]
    slot_item = ti[W + 2 * J:W + 2 * J + W * E].reshape(W, E)
    src = ti[W + 2 * J + W * E:]
    job_goff, slot_out, wave_pts = tl[:J], tl[J:J + W * E].reshape(W, E), tl[J + W * E:]
    assert src.size == got["grids"].size == int(job_ng.sum()) and np.array_equal(job_goff, np.cumsum(np.r_[0, job_ng])[:-1])
    live = slot_item >= 0
    assert np.all(live[:, 0]) and np.all(slot_out[~live] == 0)                   # slot 0 of every wave is live
    has_times = np.flatnonzero(np.diff(toff) > 0)
    assert np.array_equal(np.sort(slot_item[live]), has_times)                   # every item with times once
    assert np.array_equal(slot_out[live], toff[slot_item[live]] - toff[0])
    covered = np.concatenate([np.arange(o, o + toff[i + 1] - toff[i]) for i, o in zip(slot_item[live], slot_out[live])])
    assert np.array_equal(np.sort(covered), np.arange(T))                        # slot_out covers [0, T) in item blocks
    for w in range(W):                                                           # a wave's items share its job's series and times
        j = wave_job[w]
        for i in slot_item[w][live[w]]:
            assert series[i] == job_series[j] and job_ng[j] == SM_NSER[series[i]] + toff[i + 1] - toff[i]
            g = got["grids"][job_goff[j]:job_goff[j] + job_ng[j]]
            s = src[job_goff[j]:job_goff[j] + job_ng[j]]
            assert np.array_equal(g[s < 0], np.sort(tout[toff[i]:toff[i + 1]]))
    chunk0 = got["chunk0"]
    assert chunk0[0] == 0 and chunk0[-1] == W and np.all(np.diff(chunk0) > 0)
    pts_max = 0
    for a, b in zip(chunk0[:-1], chunk0[1:]):
        ng = job_ng[wave_job[a:b]]
        assert np.array_equal(wave_pts[a:b], np.cumsum(np.r_[0, ng])[:-1])       # wave_pts restarts at each chunk
        assert ref.smooth_wave_bytes(G, 1) * int(ng.sum()) <= ref.SMOOTH_SCRATCH_CAP
        pts_max = max(pts_max, int(ng.sum()))
    assert int(got["pts_max"][0]) == pts_max
    assert chunk0.size == (W + 1 if forced else 2)                               # a forced chunk of E models: one wave per chunk
