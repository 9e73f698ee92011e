"""Shared pieces of the bands-sampler tests (tests/test_mband_pt_cpu.py, tests/test_gpu_mband_pt.py): the log-density of a chain on
the host (the CPU build of the lane filter plus the sampler's band box) and the reference-ladder run on the lag-recovery problem,
computed once per process.  Test code only."""
import functools

import numpy as np

import mband_build as mb
import mband_pt_build as pb
import mband_ref as R


def prior3(bands):
    """(max_stdev, max_freq, min_freq) as CarmaBandsModel.context() sets them from band 0."""
    t, y, _ = pb.prepared(bands)[0]
    return 10.0 * np.sqrt(np.mean(y * y) - np.mean(y) ** 2), 1.0 / np.diff(t).min(), 1.0 / (t.max() - t.min())


def cpu_dens(bands, p, q, lag_bounds, box):
    """thx [n, dx] -> what K1 of the bands sampler gives: logdensity_mband_lane with the prior, -inf outside the band box."""
    bands = pb.prepared(bands)
    K, d, pr = len(bands), 3 + p + q, prior3(bands)

    def dens(thx):
        out = mb.logdensity(bands, p, q, thx, lag_bounds=lag_bounds, prior=pr, ignore_prior=False)
        out[~pb.in_box(thx, d, K, box)] = -np.inf
        return out
    return dens


def drawn_starts(bands, p, q, lag_bounds, seed, nchain, dens, rounds=4000):
    """Starting values as carma_bands_pt_start finds them: chain k keeps its first draw (round 0, 1, ...) whose log-density is
    finite.  -> (theta [nchain, dx], lp [nchain])."""
    pr = prior3(bands)
    dx = 3 + p + q + 3 * (len(bands) - 1)
    theta, lp = np.empty((nchain, dx)), np.full(nchain, -np.inf)
    todo = np.arange(nchain)
    for rnd in range(rounds):
        if todo.size == 0:
            break
        cand = np.array([pb.draw_start(bands, p, q, pr, lag_bounds, seed, k, rnd) for k in todo])
        v = dens(cand)
        ok = np.isfinite(v)
        theta[todo[ok]], lp[todo[ok]] = cand[ok], v[ok]
        todo = todo[~ok]
    assert todo.size == 0
    return theta, lp


RECOVERY_P, RECOVERY_Q, RECOVERY_LAG_BOUNDS = 2, 1, [(0.0, 8.0)]
RECOVERY_T, RECOVERY_LADDERS, RECOVERY_BURN, RECOVERY_SAMPLES, RECOVERY_THIN, RECOVERY_REF_SEED = 10, 32, 1000, 100, 4, 20240917


@functools.lru_cache(None)
def recovery_reference():
    """The reference ladder (carma_pt_core.h on the host, CPU log-density) on recovery_problem(): T = 10, 32 ladders, drawn
    starts, the default box.  -> dict(samples [32, S, dx], logposts [32, S], ladder: the Ladder after the run, start: (theta, lp))."""
    bands, _ = R.recovery_problem()
    p, q = RECOVERY_P, RECOVERY_Q
    d = 3 + p + q
    box = pb.default_box(bands)
    dens = cpu_dens(bands, p, q, RECOVERY_LAG_BOUNDS, box)
    T, L = RECOVERY_T, RECOVERY_LADDERS
    theta, lp = drawn_starts(bands, p, q, RECOVERY_LAG_BOUNDS, RECOVERY_REF_SEED, T * L, dens)
    R0 = pb.initial_factor(bands, d)
    lad = pb.Ladder(dens, d + 3, T, L, RECOVERY_BURN, RECOVERY_REF_SEED, theta, lp, np.tile(R0, (T * L, 1, 1)))
    lad.iterate(RECOVERY_BURN)
    samples, slp = lad.sample(RECOVERY_SAMPLES, RECOVERY_THIN)
    return dict(samples=samples, logposts=slp, ladder=lad, start=(theta, lp), dens=dens, box=box)
