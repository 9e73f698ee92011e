"""The host side of the sampler over a set of multi-band objects, without a GPU: carma_mband_set_pt_plan.h (the wave map of its
log-density kernel, the argument errors of its create call, the chunk size) compiled stand-alone with the host compiler
(tests/mbandset_pt/mbandset_pt_host.cpp), and the argument checks of CarmaBandsSet.run_mcmc."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "carma_pack_amd", "csrc")
SRC = os.path.join(HERE, "mbandset_pt", "mbandset_pt_host.cpp")
SO = os.path.join(HERE, "mbandset_pt", "libmbandset_pt_host.so")
_dp, _ip, _lp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_long)
CHAINS_MAX = 0x7fffffff - 64


@functools.lru_cache(None)
def host():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("carma_mband_set_pt_plan.h", "carma_mband_pt_plan.h", "carma_pt_sched.h", "carma_types.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-fPIC", "-shared",
                               "-o", SO, SRC])
    L = C.CDLL(SO)
    L.mbspt_run_waves.argtypes, L.mbspt_run_waves.restype = [C.c_long], C.c_long
    L.mbspt_grid.argtypes, L.mbspt_grid.restype = [C.c_long, C.c_long], C.c_long
    L.mbspt_wave.argtypes = [C.c_long, C.c_long, _lp]
    L.mbspt_chain.argtypes = [C.c_long, C.c_long, _lp]
    L.mbspt_check_create.argtypes = [_ip] + [C.c_int] * 7 + [_ip, _dp, _dp, C.c_char_p, C.c_int]
    L.mbspt_chunk_iters.argtypes, L.mbspt_chunk_iters.restype = [_ip, C.c_int, _ip], C.c_long
    L.mbspt_chunk_iters_single.argtypes, L.mbspt_chunk_iters_single.restype = [C.c_int], C.c_long
    return L


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def check_create(run_obj, S=4, ntemps=10, nreplicas=2, adapt_iters=5, dx=9, K=2, n0=None, band_lo=None, band_hi=None):
    """The message of mbandset_pt_check_create ("" = fine)."""
    w = np.ascontiguousarray(run_obj, dtype=np.int32)
    n0 = np.ascontiguousarray([10] * S if n0 is None else n0, dtype=np.int32)
    lo, hi = (None if v is None else np.ascontiguousarray(v, dtype=float) for v in (band_lo, band_hi))
    buf = C.create_string_buffer(1024)
    rc = host().mbspt_check_create(_ptr(w, _ip), w.size, S, ntemps, nreplicas, adapt_iters, dx, K, _ptr(n0, _ip), _ptr(lo, _dp),
                                   _ptr(hi, _dp), buf, 1024)
    msg = buf.value.decode()
    assert (rc == 0) == (msg == "")
    return msg


# ---- the wave map -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("RT", [1, 10, 63, 64, 65, 130])
def test_wave_map_serves_every_chain_once_and_keeps_a_wave_in_one_run(RT, M):
    L = host()
    W = L.mbspt_run_waves(RT)
    assert W == -(-RT // 64) and L.mbspt_grid(M, RT) == M * W
    served = np.zeros(M * RT, dtype=np.int64)
    out3, out2 = (C.c_long * 3)(), (C.c_long * 2)()
    for b in range(M * W):
        L.mbspt_wave(b, RT, out3)
        run, chain0, live = out3[0], out3[1], out3[2]
        assert run == b // W
        assert 1 <= live <= 64                               # lane 0 of every wave is live
        assert run * RT <= chain0 and chain0 + live <= (run + 1) * RT   # no wave spans two runs
        served[chain0:chain0 + live] += 1
        for lane in (0, live - 1):                           # the inverse map agrees
            L.mbspt_chain(chain0 + lane, RT, out2)
            assert (out2[0], out2[1]) == (b, lane)
    assert np.all(served == 1)
    # what the kernel derives from blockIdx.x, RT and W alone
    for b in range(M * W):
        j, w = b // W, b % W
        L.mbspt_wave(b, RT, out3)
        assert (out3[0], out3[1], out3[2]) == (j, j * RT + 64 * w, min(64, RT - 64 * w))


# ---- the create checks ----------------------------------------------------------------------------------------------------------
def test_create_argument_errors_name_the_run_and_its_object():
    runs = [3, 0, 2, 0, 1]
    assert check_create(runs) == ""
    assert check_create(runs, ntemps=64) == "" and check_create(runs, ntemps=1) == ""
    assert "at least one run" in check_create([])
    msg = check_create([3, 0, 4, 0, 1])
    assert msg.startswith("run 2 (object 4): ") and "out of range" in msg and "nobjects = 4" in msg
    assert check_create([0, -1]).startswith("run 1 (object -1): ")
    # too many chains: M R T beyond what a launch indexes (the first run that does not fit is named)
    big = np.array([1, 2] * 4, dtype=np.int32)
    msg = check_create(big, ntemps=64, nreplicas=2 ** 23)
    assert msg.startswith("run 3 (object 2): ") and "more than one launch can index" in msg and str(CHAINS_MAX) in msg
    assert check_create(big[:1], ntemps=64, nreplicas=2 ** 23) == ""
    # what the single object's check refuses, per run
    msg = check_create(runs, dx=38, K=8)
    assert msg.startswith("run 0 (object 3): ") and "37 at most" in msg
    assert check_create(runs, dx=37, K=8) == ""
    for bad in (0, 65):
        msg = check_create(runs, ntemps=bad)
        assert msg.startswith("run 0 (object 3): ") and "1 ... 64 temperatures" in msg
    assert "nreplicas < 1" in check_create(runs, nreplicas=0) and "adapt_iters < 0" in check_create(runs, adapt_iters=-1)
    # a box per run: the run with lo > hi is the one named
    lo, hi = np.tile([[-1.0, 0.0]], (5, 1, 1)), np.tile([[1.0, 2.0]], (5, 1, 1))
    assert check_create(runs, band_lo=lo, band_hi=hi) == ""
    assert "come together" in check_create(runs, band_lo=lo)
    lo[3, 0, 1] = 3.0
    msg = check_create(runs, band_lo=lo, band_hi=hi)
    assert msg.startswith("run 3 (object 0): ") and "band 1, mu" in msg and "lo <= hi" in msg
    lo[1, 0, 0] = np.nan
    assert check_create(runs, band_lo=lo, band_hi=hi).startswith("run 1 (object 0): band box of band 1, log a")
    # band 0 of a run's OWN object
    msg = check_create(runs, n0=[10, 1, 10, 10])
    assert msg.startswith("run 4 (object 1): ") and "band 0 needs at least 2 data" in msg
    assert check_create([3, 0, 2, 0], n0=[10, 1, 10, 10]) == ""


# ---- the chunk size -------------------------------------------------------------------------------------------------------------
def test_chunk_size_is_that_of_the_longest_object_among_the_runs():
    L = host()
    N = np.array([6, 20, 40, 600, 100000], dtype=np.int32)
    for runs in ([0], [3, 0, 2, 0, 1], [1, 2], [4, 0], [2, 2, 2]):
        w = np.ascontiguousarray(runs, dtype=np.int32)
        assert L.mbspt_chunk_iters(_ptr(w, _ip), w.size, _ptr(N, _ip)) == L.mbspt_chunk_iters_single(int(N[runs].max())), runs
    w = np.array([3], dtype=np.int32)
    assert L.mbspt_chunk_iters(_ptr(w, _ip), 1, _ptr(N, _ip)) == int(250000.0 / (0.45 * 600))
    w = np.array([0, 1], dtype=np.int32)
    assert L.mbspt_chunk_iters(_ptr(w, _ip), 2, _ptr(N, _ip)) == 4096


# ---- CarmaBandsSet.run_mcmc's argument checks, without a device -----------------------------------------------------------------
def test_run_mcmc_argument_errors_come_before_any_context():
    import carma_pack_amd as cpa
    rng = np.random.default_rng(3)
    K, S = 3, 4
    objs = [[(np.sort(rng.uniform(0, 50, 12 + b + s)), rng.standard_normal(12 + b + s), np.full(12 + b + s, 0.1)) for b in range(K)]
            for s in range(S)]
    st = cpa.CarmaBandsSet(objs, p=2, q=1, lag_bounds=[(-3, 3)] * (K - 1))
    st.context = lambda: pytest.fail("run_mcmc made a context before its argument checks")
    for m in st.models:
        m.context = st.context
    dx = st.dx
    with pytest.raises(ValueError, match="nsamples"):
        st.run_mcmc(0)
    with pytest.raises(ValueError, match="nreplicas"):
        st.run_mcmc(10, nreplicas=0)
    # the shape of init
    for bad in (np.zeros(dx - 1), np.zeros((S - 1, dx)), np.zeros((S, dx + 1)), np.zeros((1, S, dx))):
        with pytest.raises(ValueError, match="init"):
            st.run_mcmc(10, init=bad)
    with pytest.raises(ValueError, match="init"):
        st.run_mcmc(10, init=np.zeros((S, dx)), which=[3, 1])
    # the shape of the bounds (one [K - 1, 2] for all, or one per object of which), and what the model's own check refuses
    with pytest.raises(ValueError, match="scale_bounds"):
        st.run_mcmc(10, scale_bounds=[(0.1, 10.0)])
    with pytest.raises(ValueError, match="scale_bounds"):
        st.run_mcmc(10, scale_bounds=np.tile([(0.1, 10.0)], (S - 1, K - 1, 1)))
    with pytest.raises(ValueError, match="scale_bounds"):
        st.run_mcmc(10, scale_bounds=[(0.1, 10.0), (2.0, 1.0)])
    with pytest.raises(ValueError, match="object 1: scale_bounds"):
        sb = np.tile([(0.1, 10.0)], (2, K - 1, 1))
        sb[1, 0, 0] = 0.0
        st.run_mcmc(10, scale_bounds=sb, which=[3, 1])
    with pytest.raises(ValueError, match="offset_bounds"):
        st.run_mcmc(10, offset_bounds=[(0.0, 1.0, 2.0)] * 2)
    with pytest.raises(ValueError, match="offset_bounds"):
        st.run_mcmc(10, offset_bounds=np.zeros((S, K, 2)))
    # which out of range
    for bad in ([0, S], [-1], [], [[0, 1]], [0.5]):
        with pytest.raises(ValueError, match="which"):
            st.run_mcmc(10, which=bad)
    with pytest.raises(ValueError, match="ntemperatures"):
        st.run_mcmc(10, ntemperatures=65)
