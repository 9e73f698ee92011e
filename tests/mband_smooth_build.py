"""Builds/loads the host harnesses of the multi-band smoother -- test code only: the CPU build of its two passes
(tests/emu/emu_mband_smooth.cpp: carma_mband_smooth.h as the gfx950 kernels compile it) and the stand-alone planner program
(tests/mband_smooth/plan_main.cpp: carma_mband_smooth_plan.h)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "carma_pack_amd", "csrc")
EMU_SRC = os.path.join(HERE, "emu", "emu_mband_smooth.cpp")
EMU_SO = os.path.join(HERE, "emu", "libcarma_emu_mband_smooth.so")
PLAN_SRC = os.path.join(HERE, "mband_smooth", "plan_main.cpp")
PLAN_EXE = os.path.join(HERE, "mband_smooth", "plan_main")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lp = C.POINTER(C.c_long)


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
    L.emu_mband_smooth.argtypes = [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _lp, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, _ip]
    return L


@functools.lru_cache(None)
def plan_exe():
    srcs = [PLAN_SRC, os.path.join(CSRC, "carma_mband_smooth_plan.h"), os.path.join(CSRC, "carma_smooth_plan.h")]
    if _stale(PLAN_EXE, srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", PLAN_EXE, PLAN_SRC])
    return PLAN_EXE


def _run(args, text=None):
    return subprocess.run([plan_exe()] + [str(a) for a in args], input=text, capture_output=True, text=True, check=True).stdout


def smooth(bands, p, q, thx, band, tout):
    """The two passes of carma_mband_smooth.h on the host for every row of thx -> (mean [B, M], var [B, M], invalid [B]).
    bands: [(t, y, yerr)], sorted, no duplicate times within a band."""
    from mband_ref import flat
    K = len(bands)
    t, y, e, off = flat(bands)
    thx = np.ascontiguousarray(np.atleast_2d(thx), dtype=float)
    assert thx.shape[1] == 3 + p + q + 3 * (K - 1)
    tout = np.ascontiguousarray(tout, dtype=float)
    B, M = thx.shape[0], tout.size
    mean, var, inv = np.full((B, M), np.nan), np.full((B, M), np.nan), np.zeros(B, dtype=np.int32)
    rc = emu().emu_mband_smooth(p, q, K, _p(t), _p(y), _p(e), _p(off, _lp), _p(thx), B, int(band), _p(tout), M, _p(mean), _p(var),
                                _p(inv, _ip))
    assert rc == 0, rc
    return mean, var, inv


def plan_times(tout, t0):
    """mband_smooth_times -> (perm [M], rec [M + 1, 4])"""
    tout = np.asarray(tout, dtype=float)
    out = _run(["times", repr(float(t0))], "%d\n%s\n" % (tout.size, " ".join(repr(float(v)) for v in tout))).split("\n")
    return np.array(out[0].split(), dtype=int), np.array(out[1].split(), dtype=float).reshape(-1, 4)


def plan_strides(p, ng):
    return dict(zip(("fields", "fs", "ps", "ws"), (int(v) for v in _run(["strides", p, ng]).split())))


def plan_chunks(p, ng, B, forced, cap=None):
    out = _run(["chunks", p, ng, B, forced] + ([] if cap is None else [cap])).split()
    return dict(zip(("rows", "waves", "chunks", "bytes"), (int(v) for v in out)))


def plan_check(h=1, K=2, N=10, theta=1, B=1, band=0, tout=1, M=3, mean=1, var=1, bmean=0, bvar=0, bad=-1):
    """mband_smooth_check -> the message ("" = fine)"""
    return _run(["check", h, K, N, theta, B, band, tout, M, mean, var, bmean, bvar, bad]).rstrip("\n")
