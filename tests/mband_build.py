"""Builds/loads the host harnesses of the multi-band code -- test code only: the CPU build of the lane filter that merges the
bands (tests/emu/emu_mband.cpp: carma_mband.h as the gfx950 kernel compiles it) and the optimiser entry with a log-density that
calls back into Python (tests/mband/mband_mle_host.cpp: carma_mband_plan.h)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "carma_pack_amd", "csrc")
EMU_SRC = os.path.join(HERE, "emu", "emu_mband.cpp")
EMU_SO = os.path.join(HERE, "emu", "libcarma_emu_mband.so")
MLE_SRC = os.path.join(HERE, "mband", "mband_mle_host.cpp")
MLE_SO = os.path.join(HERE, "mband", "libmband_mle_host.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lp = C.POINTER(C.c_long)
DENS_CB = C.CFUNCTYPE(C.c_int, _dp, C.c_int, _dp, C.c_void_p)


def _stale(out, srcs):
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs)


def _p(a, t=_dp):
    return a.ctypes.data_as(t)


@functools.lru_cache(None)
def emu():
    srcs = [EMU_SRC, os.path.join(HERE, "emu", "grp_emu.h")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if _stale(EMU_SO, srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-mfma",
                               "-o", EMU_SO, EMU_SRC])
    L = C.CDLL(EMU_SO)
    L.emu_mband_logdensity.argtypes = [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _lp, _dp, C.c_int, _dp, _dp, C.c_int, _dp]
    return L


@functools.lru_cache(None)
def mle_host():
    deps = [MLE_SRC, os.path.join(ROOT, "include", "carma_mi355.h")] + [os.path.join(CSRC, f) for f in (
        "carma_mband_plan.h", "carma_prep.h", "carma_types.h", "carma_mle_loop.h")]
    if _stale(MLE_SO, deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-fPIC", "-shared",
                               "-o", MLE_SO, MLE_SRC])
    L = C.CDLL(MLE_SO)
    L.mband_mle_host.argtypes = [DENS_CB, C.c_void_p, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, _dp, C.c_int, C.c_int, C.c_double,
                                 C.c_double, C.c_double, _dp, _dp, _ip, _ip, _ip]
    L.mband_check_create_host.argtypes = [_dp, _dp, _dp, _lp, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_char_p, C.c_int]
    return L


def logdensity(bands, p, q, thx, lag_bounds=None, prior=(1e300, 1e300, 0.0), ignore_prior=True):
    """logdensity_mband_lane<p> on the host for every row of thx.  bands: [(t, y, yerr)], sorted, no duplicate times within a
    band; lag_bounds: [K - 1] (lo, hi); prior: max_stdev, max_freq, min_freq."""
    from mband_ref import flat
    K = len(bands)
    t, y, e, off = flat(bands)
    thx = np.ascontiguousarray(np.atleast_2d(thx), dtype=float)
    assert thx.shape[1] == 3 + p + q + 3 * (K - 1)
    lb = np.ascontiguousarray(np.zeros((max(K - 1, 1), 2)) if lag_bounds is None else np.asarray(lag_bounds, dtype=float).reshape(-1, 2))
    pr = np.array(list(prior) + [50.0])
    out = np.empty(thx.shape[0])
    rc = emu().emu_mband_logdensity(p, q, K, _p(t), _p(y), _p(e), _p(off, _lp), _p(thx), thx.shape[0], _p(lb), _p(pr),
                                    int(bool(ignore_prior)), _p(out))
    assert rc == 0, rc
    return out


def mle(fun, d, K, x0, lo, hi, fixed_lag=None, maxiter=2000, mem=8, ftol=2.220446049250313e-09, gtol=1e-5, fd_step=1e-6):
    """mband_mle_run on fun(thx [n, dx]) -> log-densities [n].  Returns (x [B, dx], f [B], status [B], calls): calls = every
    [n, dx] array of extended vectors the evaluator handed to the log-density, in order."""
    dx = d + 3 * (K - 1)
    x0 = np.ascontiguousarray(np.atleast_2d(x0), dtype=float)
    B = x0.shape[0]
    assert x0.shape[1] == dx
    lo, hi = np.ascontiguousarray(lo, dtype=float).reshape(dx), np.ascontiguousarray(hi, dtype=float).reshape(dx)
    fl = None if fixed_lag is None else np.ascontiguousarray(fixed_lag, dtype=float).reshape(B, K - 1)
    calls, err = [], []

    def cb(thx, npts, out, user):
        try:
            pts = np.ctypeslib.as_array(thx, shape=(npts, dx)).copy()
            calls.append(pts)
            np.ctypeslib.as_array(out, shape=(npts,))[:] = np.asarray(fun(pts), dtype=float).reshape(npts)
            return 0
        except BaseException as ex:                          # an exception must not cross the C frames
            err.append(ex)
            return -5

    x, f = np.full((B, dx), np.nan), np.full(B, np.nan)
    nit, nfev, status = (np.full(B, -1, dtype=np.int32) for _ in range(3))
    keep = DENS_CB(cb)
    rc = mle_host().mband_mle_host(keep, None, d, K, _p(x0), B, _p(lo), _p(hi), None if fl is None else _p(fl), int(maxiter), int(mem),
                                   float(ftol), float(gtol), float(fd_step), _p(x), _p(f), _p(nit, _ip), _p(nfev, _ip),
                                   _p(status, _ip))
    if err:
        raise err[0]
    assert rc == 0, "mband_mle_run returned %d" % rc
    return x, f, status, calls
