"""CPU side of the device-primitive tests (tests/test_gpu_device_primitives.py): the harness cross-compiles for gfx950, and the
references those tests use are themselves right -- the HOST build of carma_math.h meets every bound on exactly the arrays the
device is given (and yields the host maxima the device bounds are derived from, devprim_ref.HOST_MAX); the numpy butterfly and
row restatements equal the lane emulator (tests/emu/grp_emu.h) bit for bit; the Python Philox gives the published vectors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import devprim_ref as R


def test_harness_cross_compiles_for_gfx950(tmp_path):
    """A change of a csrc header that breaks tests/devprim/devprim.hip is seen without a GPU."""
    if not os.path.exists(R.HIPCC):
        pytest.skip("no hipcc")
    so = R.build_device(force=True, out=str(tmp_path / "libdevprim.so"))
    # (not loaded here: that would map a HIP runtime into the test process ahead of the product's own choice)
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True, timeout=60).stdout
    for sym in ("devprim_device_count", "devprim_math", "devprim_grp", "devprim_row", "devprim_philox", "devprim_rng"):
        assert " T %s\n" % sym in syms, sym


def _report(kind, mx):
    print("host maxima, %s: %s" % (kind, ", ".join("%s %.3f" % kv for kv in sorted(mx.items()))))


def test_host_math_random_arguments():
    """Set (a) and the second EXACT set through the host build: within the recorded host maxima, which lie inside what the
    project states (exp_neg_tab < 2.0, cexp_step_tab < 3.6, exp_neg and sincos_cw < 2, cexp_step <= cexp_step_tab + 0.25)."""
    mx, _ = R.measure_random("host")
    _report("random", mx)
    for name, worst in mx.items():
        assert worst <= R.HOST_MAX["random"][name], (name, worst)
        if name in R.STATED:
            assert R.HOST_MAX["random"][name] < R.STATED[name]
    assert mx["cexp"] <= mx["cexp_tab"] + 0.25


def test_host_math_edges():
    """Set (b): every edge argument; exp(-inf) gives 0 or the documented NaN / inf, never a finite non-zero value."""
    mx, minf, _ = R.measure_edges("host")
    _report("edges", mx)
    for name, worst in mx.items():
        assert worst <= R.HOST_MAX["edges"][name], (name, worst)
    assert all(minf.values()), minf


def test_host_math_slow_lane():
    """Set (c): the lane beyond the fast range (library reduction) of each complex form."""
    mx = R.measure_slow("host")
    _report("slow lane", mx)
    for name, worst in mx.items():
        assert worst <= R.HOST_MAX["slow"][name], (name, worst)


def test_exact_forms_need_the_exact_reference():
    """The two contracts differ by far more than the bounds where the phase is large: the plain form misses the exact-product
    reference of the second EXACT set by thousands of units -- so the EXACT tests do test the recovery of the rounding."""
    ta = R.big_phase_triples(9.0e4)
    re, im = R.run_math("cexp_tab", ta[0], ta[1], ta[2], on="host")
    assert R.cerr_units(re, im, R.big_phase_refs()["tab"]).max() > 1000.0


@pytest.mark.parametrize("G", [2, 4, 8, 16])
def test_butterfly_restatement_equals_the_emulator(G):
    import emu_build
    L = emu_build.lib()
    v, _ = R.grp_inputs(64, 5 + G)
    want = R.butterfly(v[:, 0], G, np.add)
    got = np.empty(64)
    L.emu_grp_sum.argtypes = [C.c_int, R._dp, R._dp]
    for g0 in range(0, 64, G):
        x = np.ascontiguousarray(v[g0:g0 + G, 0])
        o = np.empty(G)
        assert L.emu_grp_sum(G, R._ptr(x), R._ptr(o)) == 0
        got[g0:g0 + G] = o
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert all(np.unique(want[g0:g0 + G].view(np.uint64)).size == 1 for g0 in range(0, 64, G))


@pytest.mark.parametrize("P", [2, 3, 4, 5, 6, 7])
def test_row_colmix_restatement_equals_the_emulator(P):
    import emu_build
    L = emu_build.lib()
    L.emu_row_colmix.argtypes = [C.c_int, R._dp, R._dp, R._dp, R._dp]
    x = R.row_inputs(16, 40 + P)
    c, s = np.ascontiguousarray(x[:, R.RI["c"]]), np.ascontiguousarray(x[:, R.RI["s"]])
    D = np.ascontiguousarray(x[:, R.RI["D"]:R.RI["D"] + P])
    mm = np.empty((16, P))
    assert L.emu_row_colmix(P, R._ptr(c), R._ptr(s), R._ptr(D), R._ptr(mm)) == 0
    want = R.row_colmix_ref(P, c, s, D)
    assert np.array_equal(mm.view(np.uint64), want.view(np.uint64))


def test_fma_restatement_rounds_once():
    assert R.fma(1.0 + 2.0 ** -52, 1.0 + 2.0 ** -52, -1.0) == 2.0 ** -51 + 2.0 ** -104
    assert R.fma(0.1, 10.0, -1.0) == 2.0 ** -54


def test_python_philox_gives_the_published_vectors():
    from carma_pack_amd import parallel as par
    for words, want in R.PHILOX_KAT:
        assert par.philox4x32_10(*words) == want
    # (k + 0.5) 2^-53 is exact only while k + 0.5 is a double, k < 2^52; the one word pair with k = 2^53 - 1 rounds to 1.0 in
    # the device's arithmetic as in this restatement (probability 2^-53 per draw: NOTEBOOK.md, "Device primitives")
    assert 0.0 < R.u01_ref(0, 0) < R.u01_ref(0xffffffff, 0xfffff000) < 1.0
