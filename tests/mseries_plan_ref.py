"""Numpy restatement of the launch plans of the multi-series calls (carma_pack_amd/csrc/carma_mseries_plan.h) -- test yardstick
only, written from the header's comments: sorts are np.argsort(kind="stable"), tables are built whole rather than item by item.
Every function returns a dict of int64 arrays (scalars as plain ints) under the names tests/mseries/plan_main.cpp prints."""
import numpy as np

from smooth_ref import merged_grid

SMOOTH_SCRATCH_CAP = 256 << 20


def _i(a):
    return np.asarray(a, dtype=np.int64).reshape(-1)


def smooth_wave_bytes(G, ng):
    return ng * (64 * 32 + (64 // G) * 32) if G else ng * 64 * 40


def check_toff(toff):
    """-1: fine; -2: toff[0] < 0; else the first item whose times end before they start"""
    toff = _i(toff)
    if toff[0] < 0:
        return -2
    down = np.flatnonzero(np.diff(toff) < 0)
    return int(down[0]) if down.size else -1


def bucket(series, S):
    series = _i(series)
    cnt = np.bincount(series, minlength=S)
    first = np.concatenate([[0], np.cumsum(cnt)])
    return cnt, first, np.argsort(series, kind="stable")


def logdens(series, nser, repdt):
    """waves of 64 evaluations of one series; irregular-cadence series first, then longest first, ties in series order"""
    series, nser, repdt = _i(series), _i(nser), _i(repdt)
    S = nser.size
    out_of_range = np.flatnonzero((series < 0) | (series >= S))
    if out_of_range.size:
        return {"bad": int(out_of_range[0])}
    cnt, first, order = bucket(series, S)
    used = np.flatnonzero(cnt)
    used = used[np.argsort(-nser[used], kind="stable")]
    used = used[np.argsort(repdt[used] != 0, kind="stable")]
    waves = -(-cnt // 64)
    wave_series, rows = [], []
    for s in used:
        ev = order[first[s]:first[s + 1]]
        pad = np.full(waves[s] * 64 - ev.size, -1)
        rows.append(np.concatenate([ev, pad]))
        wave_series += [s] * waves[s]
    return {"W": int(waves.sum()), "w_plain": int(waves[repdt == 0].sum()), "cnt": cnt, "first": first, "order": order, "used": used,
            "wave_series": _i(wave_series), "eval_idx": _i(np.concatenate(rows)) if rows else _i([])}


def mfilter(series, nser):
    """items longest first (stable); slot j = lane j % 64 of wave j // 64; a wave's tile is [2 n(first slot)][lanes]"""
    series, nser = _i(series), _i(nser)
    M = series.size
    n_item = nser[series]
    offs = np.concatenate([[0], np.cumsum(n_item)])
    order = np.argsort(-n_item, kind="stable")
    W = -(-M // 64)
    lanes = np.minimum(64, M - 64 * np.arange(W))
    tiles = 2 * n_item[order[::64]] * lanes
    tile_off = np.concatenate([[0], np.cumsum(tiles)])
    return {"W": W, "tile_total": int(tile_off[-1]), "nmax": int(n_item.max()), "offs": offs, "order": order,
            "tint": np.concatenate([series[order], n_item[order]]), "tlong": np.concatenate([tile_off[:-1], offs[order]])}


def predict(G, series, nser, toff):
    """G = 0: a lane per (item, time) pair in the caller's order.  G >= 2: E = 64 // G pairs a wave, a wave on one series, the
    series longest first (ties in series order), a series' items in the caller's order, idle groups -1"""
    series, nser, toff = _i(series), _i(nser), _i(toff)
    M, S = series.size, nser.size
    ntimes = np.diff(toff)
    T = int(toff[-1] - toff[0])
    pair_item = np.repeat(np.arange(M), ntimes)              # output index -> item
    if not G:
        return {"W": -(-T // 64), "T": T, "E": 64, "tint": np.concatenate([series, pair_item]), "tlong": _i([])}
    E = 64 // G
    npair = np.bincount(series, weights=ntimes, minlength=S).astype(np.int64)
    used = np.flatnonzero(npair)
    used = used[np.argsort(-nser[used], kind="stable")]
    wave_series, items, outs = [], [], []
    for s in used:
        o = np.flatnonzero(series[pair_item] == s)           # ascending output index = items in the caller's order
        nw = -(-o.size // E)
        wave_series += [s] * nw
        items.append(np.concatenate([pair_item[o], np.zeros(nw * E - o.size, dtype=np.int64)]))
        outs.append(np.concatenate([o, np.full(nw * E - o.size, -1)]))
    return {"W": len(wave_series), "T": T, "E": E, "tint": np.concatenate([_i(wave_series)] + items), "tlong": _i(np.concatenate(outs))}


def smooth(G, series, nser, t_all, toff, tout, forced):
    """jobs = runs of items with equal (series, times); waves of E items of one job; chunks under the scratch cap"""
    series, nser, toff = _i(series), _i(nser), _i(toff)
    t_all, tout = np.asarray(t_all, dtype=float), np.asarray(tout, dtype=float)
    hoff = np.concatenate([[0], np.cumsum(nser)])
    E = 64 // G if G else 64
    key = lambda i: (int(series[i]), int(toff[i + 1] - toff[i]), tuple(tout[toff[i]:toff[i + 1]]))
    items = sorted((i for i in range(series.size) if toff[i + 1] > toff[i]), key=key)     # (sorted() is stable)
    wave_job, job_series, job_ng, job_goff, slot_item, slot_out, srcs, grids = [], [], [], [], [], [], [], []
    k = 0
    while k < len(items):
        k1 = k
        while k1 < len(items) and key(items[k1]) == key(items[k]):
            k1 += 1
        i0 = items[k]
        s = int(series[i0])
        grid, _, _, src = merged_grid(t_all[hoff[s]:hoff[s + 1]], tout[toff[i0]:toff[i0 + 1]])
        job_goff.append(sum(len(g) for g in grids))
        job_series.append(s)
        job_ng.append(grid.size)
        grids.append(grid)
        srcs.append(src)
        members = items[k:k1]
        nw = -(-len(members) // E)
        wave_job += [len(job_series) - 1] * nw
        slot_item += members + [-1] * (nw * E - len(members))
        slot_out += [int(toff[i] - toff[0]) for i in members] + [0] * (nw * E - len(members))
        k = k1
    W = len(wave_job)
    wmax = -(-forced // E) if forced > 0 else W
    wave_pts, chunk0, pts, nw, pts_max = [], [], 0, 0, 0
    for w in range(W):
        ng = job_ng[wave_job[w]]
        if w == 0 or nw >= wmax or smooth_wave_bytes(G, 1) * (pts + ng) > SMOOTH_SCRATCH_CAP:
            chunk0.append(w)
            pts = nw = 0
        wave_pts.append(pts)
        pts += ng
        nw += 1
        pts_max = max(pts_max, pts)
    chunk0.append(W)
    return {"E": E, "W": W, "J": len(job_series), "pts_max": pts_max, "chunk0": _i(chunk0),
            "tint": np.concatenate([_i(wave_job), _i(job_series), _i(job_ng), _i(slot_item)] + [_i(x) for x in srcs]),
            "tlong": np.concatenate([_i(job_goff), _i(slot_out), _i(wave_pts)]),
            "grids": np.concatenate(grids) if grids else np.zeros(0)}
