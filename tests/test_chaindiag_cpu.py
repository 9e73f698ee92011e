"""CPU-only: the chain diagnostics (carma_chain_diag: acor autocorrelation time, effective sample size, split R-hat) as far as
they go without a device -- the symbols, every argument error of the C entry point, the shape checks of the Python layer, "no
CPU fallback", the numpy restatement tests/chaindiag_ref.py on answers known in closed form, and the host-only level / workspace
planner carma_chaindiag_plan.h through the stand-alone program tests/chaindiag/plan_main.cpp (built and run here WITHOUT
sanitizers; a sanitizer build of it is a matter for the command line)."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import chaindiag_ref as cr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "carma_pack_amd", "csrc")
MAIN_SRC = os.path.join(HERE, "chaindiag", "plan_main.cpp")
MAIN_EXE = os.path.join(HERE, "chaindiag", "plan_main")
PLAN_H = os.path.join(CSRC, "carma_chaindiag_plan.h")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
EINVAL, ENODEV = -22, -19


def _lib():
    import carma_pack_amd._lib as L
    return L


# ---- symbols ------------------------------------------------------------------------------------
def test_symbols_exported_declared_and_listed():
    L = _lib()
    txt = open(os.path.join(ROOT, "include", "carma_mi355.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    dll = C.CDLL(L.LIB_PATH)
    for s in ("carma_chain_diag", "carma_chain_diag_dmax", "carma_chain_diag_kernel_ms"):
        assert hasattr(dll, s)
        assert re.search(r"\b%s\s*\(" % s, txt), "%s is not declared in the header" % s
        assert s in L.EXPORTS
        assert getattr(L.lib, s).argtypes is not None
    assert L.chain_diag_dmax() >= 16 == 3 + 7 + 6


# ---- argument errors of the C entry point ---------------------------------------------------------
def _call(x, G, R, Ln, d, tau, mean, sigma, status, rhat):
    L = _lib()
    p = lambda a: None if a is None else a.ctypes.data_as(_ip if a.dtype == np.int32 else _dp)
    return L.lib.carma_chain_diag(p(x), G, R, Ln, d, p(tau), p(mean), p(sigma), p(status), p(rhat), 0)


def _buffers(G=2, R=2, Ln=60, d=3):
    x = np.random.default_rng(0).standard_normal((G, R, Ln, d))
    outs = [np.full((G, R, d), 7.25) for _ in range(3)] + [np.full((G, R, d), 77, dtype=np.int32), np.full((G, d), 7.25)]
    return x, outs


BAD = {"null x": dict(x=None), "null tau": dict(tau=None), "null mean": dict(mean=None), "null sigma": dict(sigma=None),
       "null status": dict(status=None), "ngroups 0": dict(G=0), "ngroups < 0": dict(G=-1), "nreplicas 0": dict(R=0),
       "nreplicas < 0": dict(R=-3), "nsamples 0": dict(Ln=0), "nsamples < 0": dict(Ln=-60), "d 0": dict(d=0), "d < 0": dict(d=-1),
       "d > dmax": dict(d=None)}


@pytest.mark.parametrize("case", sorted(BAD))
def test_argument_errors_are_einval_and_leave_the_outputs_alone(case):
    L = _lib()
    x, (tau, mean, sigma, status, rhat) = _buffers()
    kw = dict(x=x, G=2, R=2, Ln=60, d=3, tau=tau, mean=mean, sigma=sigma, status=status, rhat=rhat)
    kw.update(BAD[case])
    if kw["d"] is None:
        kw["d"] = L.chain_diag_dmax() + 1
    assert _call(**kw) == EINVAL
    assert "carma_chain_diag" in L.last_error()
    for a in (tau, mean, sigma, rhat):
        assert np.all(a == 7.25)
    assert np.all(status == 77)


@pytest.mark.parametrize("with_rhat", [True, False])
@pytest.mark.parametrize("Ln", [1, 49, 60])
def test_a_well_formed_call_is_ok_or_enodev(Ln, with_rhat):
    """Short chains are no argument error; rhat may be NULL."""
    L = _lib()
    x, (tau, mean, sigma, status, rhat) = _buffers(Ln=Ln)
    rc = _call(x, 2, 2, Ln, 3, tau, mean, sigma, status, rhat if with_rhat else None)
    assert rc == (0 if L.lib.carma_device_count() > 0 else ENODEV), L.last_error()


# ---- the Python layer -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(), (0,), (5, 0), (2, 0, 3), (0, 2, 60, 3), (2, 2, 60, 0), (1, 1, 1, 60, 3)])
def test_binding_rejects_wrong_rank_and_empty_axes(shape):
    with pytest.raises(ValueError):
        _lib().chain_diag(np.zeros(shape))


def _no_device():
    return _lib().lib.carma_device_count() == 0


def test_no_cpu_fallback():
    """Without a device the diagnostics raise CarmaDeviceError -- nothing is computed on the host; with one they answer."""
    import carma_pack_amd as cpa
    from carma_pack_amd.carma_pack import MCMCSample
    smp = MCMCSample()
    smp._samples["mu"] = np.random.default_rng(1).standard_normal((200, 1))
    if _no_device():
        with pytest.raises(cpa.CarmaDeviceError):
            smp.effective_samples("mu")
        with pytest.raises(cpa.CarmaDeviceError):
            smp.autocorr_timescale(smp._samples["mu"][:, 0] + 0j)
        with pytest.raises(cpa.CarmaDeviceError):
            _lib().chain_diag(np.zeros((2, 60, 3)))
    else:
        ess = smp.effective_samples("mu")
        assert ess.shape == (1,) and abs(ess[0] * cr.acor(smp._samples["mu"][:, 0]).tau / 200.0 - 1.0) < 1e-10


def test_effective_samples_unknown_name_is_a_keyerror():
    from carma_pack_amd.carma_pack import MCMCSample
    with pytest.raises(KeyError):
        MCMCSample().effective_samples("nope")
    with pytest.raises(ValueError):
        MCMCSample().autocorr_timescale(np.zeros((4, 4, 4)))


class _Run(object):
    def __init__(self, R, Ln, d):
        self.s, self.lp = np.zeros((R, Ln, d)), np.zeros((R, Ln))

    def getAllSamples(self):
        return self.s, self.lp


class _Smp(object):
    def __init__(self, R=2, Ln=60, d=6):
        self._sampler = _Run(R, Ln, d)


def test_set_diagnostics_rejects_malformed_samples():
    from carma_pack_amd import CarmaModelSet
    t = np.arange(30.0)
    ms = CarmaModelSet([(t, np.sin(t + k), np.full(30, 0.1)) for k in range(3)], p=2, q=1)
    with pytest.raises(ValueError):
        ms.diagnostics()                                   # no run yet
    with pytest.raises(ValueError):
        ms.diagnostics(samples=[_Smp(), _Smp()])           # the count
    with pytest.raises(ValueError):
        ms.diagnostics(samples=[_Smp(), _Smp(), _Smp(Ln=61)])     # sample counts differ
    with pytest.raises(ValueError):
        ms.diagnostics(samples=[_Smp(), _Smp(R=3), _Smp()])       # replica counts differ
    with pytest.raises(ValueError):
        ms.diagnostics(samples=[_Smp(d=5), _Smp(), _Smp()])       # orders differ
    if _no_device():
        import carma_pack_amd as cpa
        with pytest.raises(cpa.CarmaDeviceError):          # well formed: it gets as far as the device
            ms.diagnostics(samples=[_Smp(), _Smp(), _Smp()])


# ---- the restatement on closed-form answers -----------------------------------------------------------
def test_ref_alternating_series_exact():
    """x[i] = (-1)^i, L = 50: mean 0, C[s] = (-1)^s, D = 1 + 2 (-1 + 1 - ... ) = 1, tau = 1, sigma = sqrt(1 / 50), one level."""
    a = cr.acor((-1.0) ** np.arange(50))
    assert (a.tau, a.mean, a.sigma, a.status, a.nlevels) == (1.0, 0.0, np.sqrt(1.0 / 50.0), cr.OK, 1)
    assert a.tau_last == 1.0 and a.margin == 1.0


def test_ref_statuses():
    assert cr.acor((-1.0) ** np.arange(49)).status == cr.SHORT
    c = cr.acor(np.full(200, 2.5))
    assert c.status == cr.CONSTANT and c.mean == 2.5 and np.isnan(c.tau) and np.isnan(c.sigma)
    x = np.random.default_rng(2).standard_normal(200)
    x[17] = np.nan
    n = cr.acor(x)
    assert n.status == cr.NONFINITE and np.isnan(n.mean) and np.isnan(n.tau)
    x[17] = np.inf
    n = cr.acor(x)
    assert n.status == cr.NONFINITE and n.mean == np.inf
    # a slow chain runs out of rows before tau < 2: SHORT, not a quarter of the enclosing level's value
    s = cr.acor(np.cumsum(np.ones(400)) % 200.0)           # a sawtooth of period 200
    assert s.status == cr.SHORT and s.nlevels > 1 and np.isnan(s.tau)


def test_ref_tau_is_scale_invariant_to_the_bit():
    rng = np.random.default_rng(4)
    for phi in (0.0, 0.6, 0.9):
        x = cr.ar1(rng, 2000, phi)
        a, b = cr.acor(x), cr.acor(4.0 * x)
        assert a.status == cr.OK and a.tau == b.tau and b.sigma == 4.0 * a.sigma and a.nlevels == b.nlevels
    assert cr.acor(cr.ar1(rng, 4000, 0.9)).nlevels > 1


def test_ref_rhat_of_copies():
    """R copies of one chain whose two halves coincide: every half-chain is the same, B = 0, rhat = sqrt((n - 1) / n) exactly
    as the formula rounds it."""
    h = np.random.default_rng(5).standard_normal(64)
    for R in (1, 3):
        for tail in ([], [9.0]):                          # odd L: the middle sample is dropped
            chain = np.concatenate([h, tail, h])
            n = 64
            got = cr.split_rhat(np.tile(chain, (R, 1)))
            W = np.var(h, ddof=1)
            assert got == np.sqrt(((n - 1) / n * W + 0.0) / W)
            assert abs(got - np.sqrt((n - 1) / n)) < 4e-16
    assert np.isnan(cr.split_rhat(np.zeros((2, 3))))       # n < 2
    assert np.isnan(cr.split_rhat(np.ones((2, 40))))       # W == 0
    assert cr.split_rhat(np.array([np.r_[np.zeros(20) + [0, 1] * 10, 5 + np.zeros(20) + [0, 1] * 10]])) > 3.0


# ---- the planner ----------------------------------------------------------------------------------
@functools.lru_cache(None)
def build_main():
    deps = [MAIN_SRC, PLAN_H]
    if not os.path.exists(MAIN_EXE) or any(os.path.getmtime(d) > os.path.getmtime(MAIN_EXE) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, "-o", MAIN_EXE, MAIN_SRC], check=True, timeout=300)
    return MAIN_EXE


# shapes: the thread layout, tile and halo fit the arena for every d; levels: the walk through the levels of (L, d) -- which
# are streamed, which resident, that the workspace holds every streamed one; layout: the regions of the one device block in order,
# aligned, large enough, past 2^31 bytes; limits: what one call refuses
@pytest.mark.parametrize("group", ["shapes", "levels", "layout", "limits"])
def test_planner(group):
    r = subprocess.run([build_main(), group], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "all checks met" in r.stdout


def test_the_planner_header_needs_no_hip():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-x", "c++", PLAN_H], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
