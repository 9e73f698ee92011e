"""CPU side of the device-primitive tests (tests/test_gpu_device_primitives.py): the harness cross-compiles for gfx950, and the
references those tests and tests/test_gpu_merge_primitives.py use are themselves right -- the HOST build of carma_math.h meets every bound on exactly the arrays the
device is given (and yields the host maxima the device bounds are derived from, devprim_ref.HOST_MAX); the numpy butterfly and
row restatements equal the lane emulator (tests/emu/grp_emu.h) bit for bit; the Python Philox gives the published vectors; the
float64 restatement of the merge (two_sided.merge_chol) meets the maxima the device's allowance is twice of
(devprim_ref.HOST_MAX["merge"], ["merge_real"]); a float64 run of the window block's instruction sequence, its reciprocal off by
the full 2^-24.4, lies within the running error bound of the mpmath elimination."""
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
    for sym in ("devprim_device_count", "devprim_math", "devprim_grp", "devprim_row", "devprim_philox", "devprim_rng",
                "devprim_merge", "devprim_win_init", "devprim_win_chunk", "devprim_win_chunk_masked"):
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


@pytest.mark.parametrize("P", R.MERGE_ORDERS)
def test_merge_restatement_meets_the_recorded_maxima(P):
    """two_sided.merge_chol on the synthetic families of the device test, against the closed form in mpmath: within
    HOST_MAX["merge"][P] units U = 2^-53 kappa S (the measured constant; the device test allows twice it), rank 0 within its derived
    bar (P + 2) 2^-53 S, the pivot at 4e-16 within the widened allowance.  And the closed form itself: where nothing is
    ill-conditioned (lambda_max = 0.3) it is two_sided.merge's float64 value to 1e-10 S."""
    cases, truths = R.merge_cases(P), R.merge_truths(P)
    assert len(cases) >= (P + 1) * len(R.MERGE_LAMS) * R.MERGE_DRAWS + 10
    host = np.array([R.merge_host(ev) for _, ev in cases])
    worst, worst0, err = R.merge_measure(P, host)
    print("merge_chol, P = %d, %d evaluations: largest |restatement - truth| / U %.3f; rank 0: %.3f of (P + 2) 2^-53 S" %
          (P, len(cases), worst, worst0))
    assert worst <= R.HOST_MAX["merge"][P]
    allow = R.merge_allowance(P, R.HOST_MAX["merge"][P])
    bad = [(cases[i][0], err[i], allow[i]) for i in range(len(cases)) if not err[i] <= allow[i]]
    assert not bad, bad[:5]
    ts = R._proto()
    for i, (fam, ev) in enumerate(cases):
        if fam.startswith("rank") and float(truths[i].lam) < 0.5:
            plain = ts.merge(R.lower_sym(ev[0]), ev[1], ev[2], ev[3])
            assert abs(plain - float(truths[i].value)) <= 1e-10 * float(truths[i].S), (fam, i)


@pytest.mark.parametrize("P", R.REAL_P)
def test_merge_restatement_on_real_half_filters(P):
    """merge_chol on the outputs of two_sided.half_filter, in the measure of the device test (distance from the closed form in
    mpmath relative to the whole log-likelihood): within HOST_MAX["merge_real"][P]."""
    cases = R.real_cases(P)
    want = len(R.REAL_N) * R.REAL_DRAWS if P != R.COINCIDENT[0] else 1
    assert len(cases) >= want - 2                                  # (a draw whose half filter overflows is left out)
    host = np.array([R.merge_host(ev) for _, ev in cases])
    worst = R.real_measure(P, host)
    print("merge_chol on real half filters, P = %d, %d evaluations: %.3g of the log-likelihood" % (P, len(cases), worst))
    assert worst <= R.HOST_MAX["merge_real"][P]


@pytest.mark.parametrize("P", R.MERGE_ORDERS)
def test_window_chunk_bound_holds_for_a_float64_run(P):
    """The mpmath elimination's running error bound against a float64 run of the block's own instruction sequence whose reciprocal
    is off by the full 2^-24.4, on the two kinds of chunk the device test uses: inside the bound -- and with the Newton step left
    out (t off by 2^-24.4 instead of 2^-48) far outside it, so the bound does hold t to its stated accuracy."""
    for seed, noise, gain in ((600 + P, 1.0, 0.5), (700 + P, 1e-3, 0.0)):
        x = R.win_chunk_inputs(P, seed, noise, gain)[:16]
        val, err = R.win_chunk_truth(P, x)
        assert all(float(err[l, c]) <= 1e-6 * max(1.0, abs(float(val[l, c]))) for l, c in R.win_checked(P))   # (not vacuous)
        assert all(float(val[j, P + (j & 1)]) > 0.0 for j in range(16 - P))                                   # (every variance positive)
        assert R.win_chunk_worst(P, R.win_chunk_f64(P, x), val, err) <= 1.0
        assert R.win_chunk_worst(P, R.win_chunk_f64(P, x, newton=False), val, err) > 100.0
    x = R.win_neutral_inputs(P, 800 + P)[:16]
    out = R.win_chunk_f64(P, x)
    assert np.array_equal(out[16 - P:, :P], x[16 - P:, :P]) and np.array_equal(out[16 - P:, P + 2], x[16 - P:, 2 * P + 1])


def test_window_init_restatement_is_the_sum():
    """win_init_ref: kn_r + sum_s S_rs hn_s and nun + sum_s nuF@s hn_s, to rounding."""
    P, ND = 5, 11
    x = R.win_init_inputs(P, 305)[:16]
    out = R.win_init_ref(P, x)
    S, nuF = x[ND:, P + 1:2 * P + 1].T, x[ND:, 2 * P + 1]          # S[r, s] = kk_r of lane ND + s
    for l in range(16):
        hn = x[l, 2 * P + 2:]
        assert np.allclose(out[l, :P], x[l, :P] + S @ hn, rtol=1e-12, atol=1e-12)
        assert np.isclose(out[l, P], x[l, P] + nuF @ hn, rtol=1e-12, atol=1e-12)
