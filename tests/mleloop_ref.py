"""Builds and loads the host harness of the lock-step optimiser's loop (tests/mleloop/: carma_mle_loop.h instantiated with an
evaluator that calls back into Python), runs it on a numpy objective and records every launch it makes.  Test code only."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "carma_pack_amd", "csrc")
HOST_SRC = os.path.join(HERE, "mleloop", "mleloop_host.cpp")
HOST_SO = os.path.join(HERE, "mleloop", "libmleloop_host.so")
MAIN_SRC = os.path.join(HERE, "mleloop", "mleloop_main.cpp")
MAIN_EXE = os.path.join(HERE, "mleloop", "mleloop_main")
DEPS = [os.path.join(CSRC, "carma_mle_loop.h"), os.path.join(ROOT, "include", "carma_mi355.h")]
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC]

FTOL_DEFAULT = 2.220446049250313e-09                        # the defaults of Context.mle_batched
EPS = np.finfo(float).eps

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
CALLBACK = C.CFUNCTYPE(C.c_int, _dp, _ip, C.c_int, _dp, C.c_void_p)


def _stale(out, deps):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


def build_host():
    if _stale(HOST_SO, [HOST_SRC] + DEPS):
        subprocess.run(["g++"] + FLAGS + ["-fPIC", "-shared", "-o", HOST_SO, HOST_SRC], check=True, timeout=300)
    return HOST_SO


def build_main():
    """The stand-alone program, without sanitizers."""
    if _stale(MAIN_EXE, [MAIN_SRC] + DEPS):
        subprocess.run(["g++"] + FLAGS + ["-o", MAIN_EXE, MAIN_SRC], check=True, timeout=300)
    return MAIN_EXE


@functools.lru_cache(None)
def host():
    L = C.CDLL(build_host())
    for fn in (L.mleloop_shared, L.mleloop_per_start):
        fn.argtypes = [CALLBACK, C.c_void_p, C.c_int, _dp, C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                       C.c_double, _dp, _dp, _ip, _ip, _ip]
        fn.restype = C.c_int
    L.mleloop_constants.argtypes = [_dp, _ip, _ip]
    L.mleloop_constants.restype = None
    return L


def constants():
    big, k, pat = C.c_double(), C.c_int(), C.c_int()
    host().mleloop_constants(C.byref(big), C.byref(k), C.byref(pat))
    return big.value, k.value, pat.value


class Run(object):
    """x [B, d], fun, nit, nfev, status [B]; calls: one (pts [n, d], owner [n] or None, values [n]) per launch, in order."""

    def __init__(self, x, fun, nit, nfev, status, calls):
        self.x, self.fun, self.nit, self.nfev, self.status, self.calls = x, fun, nit, nfev, status, calls

    def fmax(self):
        """Largest finite |f| any launch returned."""
        m = 0.0
        for _, _, v in self.calls:
            fin = np.isfinite(v)
            if fin.any():
                m = max(m, float(np.abs(v[fin]).max()))
        return m


def _ptr(a, t=_dp):
    return a.ctypes.data_as(t)


def minimize(fun, x0, lo, hi, per_start=False, maxiter=2000, mem=8, ftol=FTOL_DEFAULT, gtol=1e-5, fd_step=1e-6):
    """mle_loop on fun(pts [n, d], owner [n] or None) -> [n] (pointwise; non-finite = infeasible).  lo / hi: [d] (one box,
    bstride 0) or [B, d] (a box per start, bstride d); +-inf = unbounded.  per_start: the evaluator with PER_START true (owner
    is filled).  Returns a Run."""
    x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64))
    assert x0.ndim == 2
    B, d = x0.shape
    lo = np.ascontiguousarray(np.asarray(lo, dtype=np.float64))
    hi = np.ascontiguousarray(np.asarray(hi, dtype=np.float64))
    assert lo.shape == hi.shape and lo.shape in ((d,), (B, d))
    bstride = 0 if lo.ndim == 1 else d
    calls, err = [], []

    def cb(pts, owner, npts, out, user):
        try:
            p = np.ctypeslib.as_array(pts, shape=(npts, d)).copy()
            o = np.ctypeslib.as_array(owner, shape=(npts,)).copy() if owner else None
            v = np.asarray(fun(p, o), dtype=np.float64).reshape(npts)
            calls.append((p, o, v.copy()))
            np.ctypeslib.as_array(out, shape=(npts,))[:] = v
            return 0
        except BaseException as ex:                          # an exception must not cross the C frames
            err.append(ex)
            return -5

    x, f = np.full((B, d), np.nan), np.full(B, np.nan)
    nit, nfev, status = (np.full(B, -1, dtype=np.int32) for _ in range(3))
    entry = host().mleloop_per_start if per_start else host().mleloop_shared
    keep = CALLBACK(cb)
    rc = entry(keep, None, d, _ptr(x0), B, _ptr(lo), _ptr(hi), bstride, int(maxiter), int(mem), float(ftol), float(gtol),
               float(fd_step), _ptr(x), _ptr(f), _ptr(nit, _ip), _ptr(nfev, _ip), _ptr(status, _ip))
    if err:
        raise err[0]
    assert rc == 0, "mle_loop returned %d" % rc
    return Run(x, f, nit, nfev, status, calls)


# ---- the launches of a run, read back ---------------------------------------------------------------------------------------
def ks_of(nn, d, ls_k=8):
    """Candidates of the first line-search launch that carry their difference stencil (carma_mle_loop.h: KS)."""
    return max(1, min(ls_k, (1024 // nn - ls_k) // (2 * d)))


def parse_calls(run, d, ls_k=8):
    """The launches of a PER_START run, grouped by iteration, from the owners alone.  Every launch holds equally many points of
    each of its starts, in runs of equal owner; the width of a run names the launch: 2 d + 1 a gradient launch, ls_k + 2 d KS a
    first line-search round (KS from the number of starts in it), ls_k a later round.  Returns (first, iterations): the starts of
    the initial gradient launch, and per iteration a dict(ls=[starts per round], grad=starts or None)."""
    out, first = [], None
    for n, (pts, owner, _) in enumerate(run.calls):
        assert owner is not None
        cut = np.flatnonzero(np.diff(owner)) + 1
        starts = owner[np.r_[0, cut]]
        widths = np.diff(np.r_[0, cut, owner.size])
        assert np.unique(starts).size == starts.size, "launch %d: a start appears in two runs" % n
        assert np.all(widths == widths[0]), "launch %d: runs of different width %s" % (n, widths)
        w, nn = int(widths[0]), starts.size
        if n == 0:
            assert w == 2 * d + 1
            first = starts
        elif w == 2 * d + 1:
            assert out and out[-1]["grad"] is None, "launch %d: a second gradient launch in one iteration" % n
            out[-1]["grad"] = starts
        elif w == ls_k + 2 * d * ks_of(nn, d, ls_k):
            out.append(dict(ls=[starts], grad=None))
        else:
            assert w == ls_k, "launch %d: %d points per start among %d starts is no launch of the loop" % (n, w, nn)
            assert out and out[-1]["grad"] is None, "launch %d: a line-search round after the gradient launch" % n
            out[-1]["ls"].append(starts)
    return first, out
