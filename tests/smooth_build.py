"""Builds/loads the CPU lane emulator of the one-pass smoother (tests/emu/emu_smooth.cpp) and the stand-alone planner program
(tests/smooth/plan_main.cpp) -- test harness only."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "carma_pack_amd", "csrc")
SO = os.path.join(HERE, "emu", "libcarma_emu_smooth.so")
PLAN_EXE = os.path.join(HERE, "smooth", "plan_main")
_dp = C.POINTER(C.c_double)
_lib = None


def _stale(out, srcs):
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs)


def lib():
    global _lib
    if _lib is None:
        srcs = [os.path.join(HERE, "emu", "emu_smooth.cpp"), os.path.join(HERE, "emu", "grp_emu.h")]
        srcs += [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
        if _stale(SO, srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-mfma",
                                   "-o", SO, srcs[0]])
        _lib = C.CDLL(SO)
    return _lib


def plan_exe():
    srcs = [os.path.join(HERE, "smooth", "plan_main.cpp"), os.path.join(CSRC, "carma_smooth_plan.h")]
    if _stale(PLAN_EXE, srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", PLAN_EXE, srcs[0]])
    return PLAN_EXE


def plan_merge(t, tout):
    """smooth_merge of carma_smooth_plan.h -> (grid, dpos, spos, src)"""
    t, tout = np.asarray(t, dtype=float), np.asarray(tout, dtype=float)
    text = "%d %d\n%s\n%s\n" % (t.size, tout.size, " ".join(repr(float(v)) for v in t), " ".join(repr(float(v)) for v in tout))
    out = subprocess.run([plan_exe(), "merge"], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    return (np.array(out[0].split(), dtype=float), np.array(out[1].split(), dtype=int), np.array(out[2].split(), dtype=int),
            np.array(out[3].split(), dtype=int))


def plan_chunks(G, ng, K, forced):
    """smooth_chunks -> dict(E, models, waves, rec_elems, grp_elems, bytes)"""
    out = subprocess.run([plan_exe(), "chunks", str(G), str(ng), str(K), str(forced)], capture_output=True, text=True,
                         check=True).stdout.split()
    return dict(zip(("E", "models", "waves", "rec_elems", "grp_elems", "bytes"), (int(v) for v in out)))


def _p(a):
    return a.ctypes.data_as(_dp)


def _series(t, y, yerr):
    s = np.zeros((t.size, 4))
    s[1:, 0] = np.diff(t)
    s[:, 1] = y
    s[:, 2] = yerr ** 2
    s[:, 3] = t
    return s


def smooth_carma(t, y, yerr, sigsqr, roots, ma, tout, mu=0.0):
    """smooth_forward / smooth_backward <P, G> on the lane emulator (roots: conjugate pairs adjacent, as the C ABI normalises)."""
    roots = np.asarray(roots, dtype=complex)
    p = roots.size
    om = np.ascontiguousarray(np.c_[roots.real, roots.imag])
    mac = np.zeros(p)
    mac[:np.size(ma)] = ma
    s = _series(np.asarray(t, float), np.asarray(y, float), np.asarray(yerr, float))
    tout = np.ascontiguousarray(tout, dtype=float)
    mean, var = np.empty(tout.size), np.empty(tout.size)
    rc = lib().emu_smooth_carma(p, _p(om), _p(mac), C.c_double(sigsqr), C.c_double(mu), _p(s), s.shape[0], _p(tout), tout.size,
                                _p(mean), _p(var))
    assert rc == 0, rc
    return mean, var


def smooth_car1(t, y, yerr, sigsqr, omega, tout, mu=0.0):
    s = _series(np.asarray(t, float), np.asarray(y, float), np.asarray(yerr, float))
    tout = np.ascontiguousarray(tout, dtype=float)
    mean, var = np.empty(tout.size), np.empty(tout.size)
    lib().emu_smooth_car1(C.c_double(sigsqr), C.c_double(omega), C.c_double(mu), _p(s), s.shape[0], _p(tout), tout.size, _p(mean),
                          _p(var))
    return mean, var
