"""Builds/loads the host harness of the calls on a set of multi-band objects -- test code only: the create checks, the per-start
boxes, the launch plan and the lock-step optimiser of carma_mband_set_plan.h with a log-density that calls back into Python
(tests/mbandset/mbandset_host.cpp)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "carma_pack_amd", "csrc")
SRC = os.path.join(HERE, "mbandset", "mbandset_host.cpp")
SO = os.path.join(HERE, "mbandset", "libmbandset_host.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lp = C.POINTER(C.c_long)
DENS_CB = C.CFUNCTYPE(C.c_int, _dp, _ip, C.c_int, _dp, C.c_void_p)


def _p(a, t=_dp):
    return None if a is None else a.ctypes.data_as(t)


@functools.lru_cache(None)
def host():
    deps = [SRC, os.path.join(ROOT, "include", "carma_mi355.h")] + [os.path.join(CSRC, f) for f in (
        "carma_mband_set_plan.h", "carma_mband_plan.h", "carma_prep.h", "carma_types.h", "carma_mle_loop.h", "carma_mseries_plan.h",
        "carma_smooth_plan.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-fPIC", "-shared",
                               "-o", SO, SRC])
    L = C.CDLL(SO)
    L.mbandset_check_create_host.argtypes = [_dp, _dp, _dp, _lp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_char_p, C.c_int]
    L.mbandset_cut_boxes_host.argtypes = [_dp, _dp, _ip, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _ip]
    L.mbandset_cut_boxes_host.restype = C.c_long
    L.mbandset_mle_host.argtypes = [DENS_CB, C.c_void_p, C.c_int, C.c_int, _dp, _ip, C.c_int, _dp, _dp, _dp, C.c_int, C.c_int,
                                    C.c_double, C.c_double, C.c_double, _dp, _dp, _ip, _ip, _ip]
    L.mbandset_plan_host.argtypes = [_ip, C.c_int, C.c_int, _ip, _ip, _ip, C.c_long]
    L.mbandset_plan_host.restype = C.c_long
    L.mbandset_prepared_host.argtypes = [_dp, _dp, _dp, _lp, C.c_int, C.c_int, _dp, _dp, _dp, C.c_int, C.c_int, C.c_char_p, C.c_long]
    L.mbandset_prepared_host.restype = C.c_long
    return L


def flat_set(objects):
    """(time, y, yerr, offsets [S K + 1]) as carma_bandset_create takes S objects of K bands each."""
    bands = [b for obj in objects for b in obj]
    off = np.zeros(len(bands) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(b[0]) for b in bands])
    return tuple(np.ascontiguousarray(np.concatenate([np.asarray(b[k], dtype=float) for b in bands])) for k in range(3)) + (off,)


def check_create(time, y, yerr, offsets, S, K, p, q, lag_lo, lag_hi):
    """mbandset_check_create: "" or the message."""
    time, y, yerr = (np.ascontiguousarray(a, dtype=float) for a in (time, y, yerr))
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    lo, hi = (None if a is None else np.ascontiguousarray(a, dtype=float) for a in (lag_lo, lag_hi))
    msg = C.create_string_buffer(512)
    rc = host().mbandset_check_create_host(_p(time), _p(y), _p(yerr), _p(offsets, _lp), S, K, p, q, _p(lo), _p(hi), msg, 512)
    assert (rc == 0) == (msg.value == b"")
    return msg.value.decode()


def prepared(objects, lag_lo, lag_hi, max_stdev, s, alone):
    """The bytes the preparation leaves of object s (records, boff, n, N, lagbox, the three prior numbers): its slice of the set
    prepared as a whole, or -- alone -- the object prepared on its own as carma_bands_create gets it.  max_stdev: [S] or None."""
    t, y, e, off = flat_set(objects)
    S, K = len(objects), len(objects[0])
    lo, hi = (np.ascontiguousarray(a, dtype=float).reshape(S, K - 1) for a in (lag_lo, lag_hi))
    ms = None if max_stdev is None else np.ascontiguousarray(max_stdev, dtype=float).reshape(S)
    buf = C.create_string_buffer(1 << 16)
    nb = host().mbandset_prepared_host(_p(t), _p(y), _p(e), _p(off, _lp), S, K, _p(lo), _p(hi), _p(ms), s, int(alone), buf, len(buf))
    assert nb > 0, nb
    return buf.raw[:nb]


def cut_boxes(lo, hi, which, d, K, lagbox, fixed=False):
    """mbandset_cut_boxes on copies: (lo, hi, bad start or -1, band)."""
    lo, hi = (np.array(a, dtype=float, order="C") for a in (lo, hi))
    which = np.ascontiguousarray(which, dtype=np.int32)
    lagbox = np.ascontiguousarray(lagbox, dtype=float)
    band = np.zeros(1, dtype=np.int32)
    bad = host().mbandset_cut_boxes_host(_p(lo), _p(hi), _p(which, _ip), which.size, d, K, _p(lagbox), int(fixed), _p(band, _ip))
    return lo, hi, int(bad), int(band[0])


def plan(which, N):
    """The launch plan of evaluations on objects `which` with N[s] data: (wave_obj [W], eval_idx [W, 64])."""
    which = np.ascontiguousarray(which, dtype=np.int32)
    N = np.ascontiguousarray(N, dtype=np.int32)
    W = host().mbandset_plan_host(_p(which, _ip), which.size, N.size, _p(N, _ip), None, None, -1)
    if W < 0:
        raise ValueError("object[%d] out of range" % (-2 - W))
    wobj, eidx = np.full(max(W, 1), -7, dtype=np.int32), np.full((max(W, 1), 64), -7, dtype=np.int32)
    assert host().mbandset_plan_host(_p(which, _ip), which.size, N.size, _p(N, _ip), _p(wobj, _ip), _p(eidx, _ip), W) == W
    return wobj[:W], eidx[:W]


def mle(fun, d, K, x0, which, lo, hi, fixed_lag=None, maxiter=2000, mem=8, ftol=2.220446049250313e-09, gtol=1e-5, fd_step=1e-6):
    """mbandset_mle_run on fun(thx [n, dx], object [n]) -> log-densities [n].  Returns (x [B, dx], f [B], nit [B], status [B],
    calls): calls = every (thx [n, dx], object [n]) the evaluator handed to the log-density, in order."""
    dx = d + 3 * (K - 1)
    x0 = np.ascontiguousarray(np.atleast_2d(x0), dtype=float)
    B = x0.shape[0]
    assert x0.shape[1] == dx
    which = np.ascontiguousarray(which, dtype=np.int32).reshape(B)
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=float), (B, dx)))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=float), (B, dx)))
    fl = None if fixed_lag is None else np.ascontiguousarray(fixed_lag, dtype=float).reshape(B, K - 1)
    calls, err = [], []

    def cb(thx, obj, npts, out, user):
        try:
            pts = np.ctypeslib.as_array(thx, shape=(npts, dx)).copy()
            ob = np.ctypeslib.as_array(obj, shape=(npts,)).copy()
            calls.append((pts, ob))
            np.ctypeslib.as_array(out, shape=(npts,))[:] = np.asarray(fun(pts, ob), dtype=float).reshape(npts)
            return 0
        except BaseException as ex:                          # an exception must not cross the C frames
            err.append(ex)
            return -5

    x, f = np.full((B, dx), np.nan), np.full(B, np.nan)
    nit, nfev, status = (np.full(B, -1, dtype=np.int32) for _ in range(3))
    keep = DENS_CB(cb)
    rc = host().mbandset_mle_host(keep, None, d, K, _p(x0), _p(which, _ip), B, _p(lo), _p(hi), _p(fl), int(maxiter), int(mem),
                                  float(ftol), float(gtol), float(fd_step), _p(x), _p(f), _p(nit, _ip), _p(nfev, _ip),
                                  _p(status, _ip))
    if err:
        raise err[0]
    assert rc == 0, "mbandset_mle_run returned %d" % rc
    return x, f, nit, status, calls
