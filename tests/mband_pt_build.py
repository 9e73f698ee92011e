"""Builds/loads the host harnesses of the bands sampler -- test code only: the reference ladder (tests/emu/emu_pt_generic.cpp:
ram_propose / ram_finish / exchange_sweep of carma_pt_core.h at any dimension, the log-density a Python callback) and the host-only
decisions of carma_mband_pt_plan.h with the RAM-kernel planner of carma_shape_plan.h (tests/mbandpt/mband_pt_plan_host.cpp)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from mband_build import DENS_CB, _p, _stale

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "carma_pack_amd", "csrc")
EMU_SRC = os.path.join(HERE, "emu", "emu_pt_generic.cpp")
EMU_SO = os.path.join(HERE, "emu", "libcarma_emu_pt_generic.so")
PLAN_SRC = os.path.join(HERE, "mbandpt", "mband_pt_plan_host.cpp")
PLAN_SO = os.path.join(HERE, "mbandpt", "libmband_pt_plan_host.so")
_dp, _ip, _lp, _up = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_uint)
RAM_NONE, RAM_FUSED, RAM_SPLIT, RAM_WIDE = 0, 1, 2, 3


@functools.lru_cache(None)
def emu():
    srcs = [EMU_SRC, os.path.join(HERE, "emu", "grp_emu.h")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if _stale(EMU_SO, srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-mfma",
                               "-o", EMU_SO, EMU_SRC])
    L = C.CDLL(EMU_SO)
    L.emu_pt_generic.argtypes = [DENS_CB, C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, C.c_int, C.c_ulonglong, C.c_long, C.c_int,
                                 C.c_uint, C.c_uint, _dp, _dp, _dp, _dp, _dp, _up, _up]
    return L


@functools.lru_cache(None)
def plan():
    deps = [PLAN_SRC] + [os.path.join(CSRC, f) for f in ("carma_mband_pt_plan.h", "carma_pt_sched.h", "carma_shape_plan.h", "carma_types.h")]
    if _stale(PLAN_SO, deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-fPIC", "-shared",
                               "-o", PLAN_SO, PLAN_SRC])
    L = C.CDLL(PLAN_SO)
    L.mbpt_check_create.argtypes = [C.c_int] * 6 + [_dp, _dp, C.c_char_p, C.c_int]
    L.mbpt_initial_factor.argtypes = [_dp, _dp, _lp, C.c_int, C.c_int, _dp]
    L.mbpt_draw_start.argtypes = [_dp, _dp, _lp, C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_ulonglong, C.c_ulonglong, C.c_int, _dp]
    L.mbpt_default_box.argtypes = [_dp, _dp, _lp, C.c_int, _dp, _dp]
    L.mbpt_in_box.argtypes = [_dp, C.c_int, C.c_int, _dp, _dp]
    L.mbpt_chunk_iters.argtypes = [C.c_int]
    L.mbpt_chunk_iters.restype = C.c_long
    L.mbpt_ram_kernels_plan.argtypes = [C.c_int, C.c_int, C.c_long]
    return L


def prepared(bands):
    """The bands as the library keeps them: sorted, the first of equal times kept."""
    out = []
    for t, y, e in bands:
        t, y, e = (np.asarray(a, dtype=float) for a in (t, y, e))
        _, idx = np.unique(t, return_index=True)
        out.append((t[idx], y[idx], e[idx]))
    return out


def _flat_ty(bands):
    from mband_ref import flat
    t, y, _, off = flat(prepared(bands))
    return t, y, off


def check_create(ntemps, nreplicas, adapt_iters, dx, K, n0=10, band_lo=None, band_hi=None):
    """The message of mband_pt_check_create ("" = fine)."""
    lo = None if band_lo is None else np.ascontiguousarray(band_lo, dtype=float)
    hi = None if band_hi is None else np.ascontiguousarray(band_hi, dtype=float)
    buf = C.create_string_buffer(512)
    rc = plan().mbpt_check_create(ntemps, nreplicas, adapt_iters, dx, K, n0, None if lo is None else _p(lo), None if hi is None else _p(hi),
                                  buf, 512)
    msg = buf.value.decode()
    assert (rc == 0) == (msg == "")
    return msg


def initial_factor(bands, d):
    t, y, off = _flat_ty(bands)
    K = len(bands)
    dx = d + 3 * (K - 1)
    R0 = np.empty((dx, dx))
    plan().mbpt_initial_factor(_p(t), _p(y), _p(off, _lp), K, d, _p(R0))
    return R0


def draw_start(bands, p, q, prior3, lag_bounds, seed, chain, round_=0):
    """The starting draw of `chain` in `round_`; prior3 = (max_stdev, max_freq, min_freq) of the context."""
    t, y, off = _flat_ty(bands)
    K = len(bands)
    pr = np.array(list(prior3) + [50.0])
    lb = np.ascontiguousarray(np.asarray(lag_bounds, dtype=float).reshape(-1, 2)) if K > 1 else np.zeros((1, 2))
    out = np.empty(3 + p + q + 3 * (K - 1))
    plan().mbpt_draw_start(_p(t), _p(y), _p(off, _lp), K, _p(pr), p, q, _p(lb), int(seed), int(chain), int(round_), _p(out))
    return out


def default_box(bands):
    t, y, off = _flat_ty(bands)
    K = len(bands)
    lo, hi = np.empty((max(K - 1, 1), 2)), np.empty((max(K - 1, 1), 2))
    plan().mbpt_default_box(_p(t), _p(y), _p(off, _lp), K, _p(lo), _p(hi))
    return lo[:K - 1], hi[:K - 1]


def ram_kernels_plan(d, wide_min=None):
    return plan().mbpt_ram_kernels_plan(int(d), 0 if wide_min is None else 1, 0 if wide_min is None else int(wide_min))


def in_box(thx, d, K, box):
    """[n] bool: (log a_b, mu_b) of every band inside box = (lo, hi), [K - 1, 2] each (None: no box)."""
    thx = np.atleast_2d(thx)
    if box is None or K < 2:
        return np.ones(thx.shape[0], dtype=bool)
    lo, hi = (np.asarray(v, dtype=float).reshape(K - 1, 2) for v in box)
    cols = d + 3 * np.arange(K - 1)
    ok = np.ones(thx.shape[0], dtype=bool)
    for k in range(2):
        v = thx[:, cols + 1 + k]
        ok &= np.all((v >= lo[:, k]) & (v <= hi[:, k]), axis=1)
    return ok


class Ladder(object):
    """R ladders of T chains of dimension d advanced by emu_pt_generic.  dens(thn [nc, d]) -> [nc] log-densities.  The state
    (theta [R, T, d], lp [R, T], chol [R, T, d, d], nacc, nswap [R, T], iterations done) lives here between calls."""

    def __init__(self, dens, d, T, R, maxiter, seed, theta, lp, chol, temps=None):
        self.dens, self.d, self.T, self.R, self.maxiter, self.seed = dens, int(d), int(T), int(R), int(maxiter), int(seed)
        self.temps = np.ascontiguousarray(np.exp(np.log(100.0) * np.arange(T) / max(T - 1, 1)) if temps is None else temps, dtype=float)
        self.theta = np.array(theta, dtype=float).reshape(R, T, d).copy()
        self.lp = np.array(lp, dtype=float).reshape(R, T).copy()
        self.chol = np.array(chol, dtype=float).reshape(R, T, d, d).copy()
        self.nacc = np.zeros((R, T), dtype=np.uint32)
        self.nswap = np.zeros((R, T), dtype=np.uint32)
        self.iter = 0

    def _run(self, niter, thin):
        d, nc = self.d, self.R * self.T
        err = []

        def cb(thn, n, out, user):
            try:
                pts = np.ctypeslib.as_array(thn, shape=(n, d)).copy()
                np.ctypeslib.as_array(out, shape=(n,))[:] = np.asarray(self.dens(pts), dtype=float).reshape(n)
                return 0
            except BaseException as ex:                      # an exception must not cross the C frames
                err.append(ex)
                return -5

        ns = niter // thin if thin > 0 else 0
        samples, slp = np.full((self.R, max(ns, 1), d), np.nan), np.full((self.R, max(ns, 1)), np.nan)
        keep = DENS_CB(cb)
        rc = emu().emu_pt_generic(keep, None, d, self.T, self.R, _p(self.temps), self.maxiter, self.iter, int(niter), int(thin),
                                  self.seed & 0xffffffff, (self.seed >> 32) & 0xffffffff, _p(self.theta), _p(self.lp), _p(self.chol),
                                  _p(samples), _p(slp), _p(self.nacc, _up), _p(self.nswap, _up))
        if err:
            raise err[0]
        assert rc == 0, "emu_pt_generic returned %d" % rc
        assert nc == self.lp.size
        self.iter += int(niter)
        return samples[:, :ns], slp[:, :ns]

    def iterate(self, niter):
        self._run(niter, 0)

    def sample(self, nsamples, thin=1):
        return self._run(int(nsamples) * int(thin), int(thin))
