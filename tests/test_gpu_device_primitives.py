"""The device building blocks on their own, one primitive call per lane (tests/devprim/devprim.hip, built with the flags of
build.sh and loaded with ctypes): carma_math.h against mpmath, grp_device.h against numpy restatements bit for bit,
carma_row_asm.h against the formulas in its comments, carma_rng.h against the published Philox vectors and mpmath.
Every reference runs on the CPU (tests/devprim_ref.py; tests/test_devprim_cpu.py holds the references themselves to the host
build and the lane emulator).  After a launcher has returned a HIP error nothing more is launched: every later test fails
with "harness reported HIP error N earlier"."""
import numpy as np
import pytest

import devprim_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    L = R.device()
    assert L.devprim_device_count() >= 1
    return L


def _report(kind, mx):
    print("device maxima, %s: %s" % (kind, ", ".join("%s %.3f" % kv for kv in sorted(mx.items()))))


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _host_difference(out, host_out):
    """Largest difference between the device and the host build in units of 2^-53 of the larger output (reported)."""
    worst = {}
    for name in out:
        d = 0.0
        for k in range(2):
            g, h = out[name][k], host_out[name][k]
            fin = np.isfinite(g) & np.isfinite(h)
            scale = np.maximum(np.maximum(np.abs(out[name][0]), np.abs(out[name][1])), R.TINY / R.U53) * R.U53
            if fin.any():
                d = max(d, float((np.abs(g - h) / scale)[fin].max()))
        worst[name] = d
    return worst


# Device maxima of the first run on an MI355X (NOTEBOOK.md, "Device primitives"):
#                 exp_neg exp_neg_tab sincos_cw  cexp   cexp_tab cexp_exact cexp_tab_exact big_poly_exact big_tab_exact
#   random         1.139     1.738      1.382    2.974   2.974     3.086       3.066          3.330         2.830
#   edges          0.983     1.266      0.959    2.126   1.431     2.126       1.431
#   slow lane                                    0.676   0.794     1.162       1.115
def test_math_random_arguments(dev):
    """(a) 20 000 triples of the distribution of table_math_accuracy.cpp, every one compared.  Bounds (devprim_ref.STATED,
    HOST_MAX): exp_neg < 2.0 (host 1.14), exp_neg_tab < 2.0 (host 1.74), sincos_cw < 2 (host 1.39), cexp_step_tab < 3.6
    (host 2.98), cexp_step <= cexp_step_tab + 0.25 and < 3.85 (host 2.98); host maximum + 1 for what nobody had measured:
    cexp_step<true> 3.09 -> 4.09, cexp_step_tab<true> 3.07 -> 4.07, and on the second EXACT set (|b dt| in [1e3, 1e6) /
    [1e3, 9e4)) 3.34 -> 4.34 and 2.84 -> 3.84: the error does not grow with the phase."""
    mx, out = R.measure_random("device")
    _report("random", mx)
    # the first run on an MI355X found the device bit-identical to the host build (g++ -mfma, glibc) on every fast path: the
    # same FMA sequences, and rint / ldexp agree.  Held from then on (the library slow path and the edges are not).
    _, host_out = R.measure_random("host")
    print("largest device - host difference (units of 2^-53 of |rho|):", _host_difference(out, host_out))
    for name in out:
        for k in range(2):
            assert np.array_equal(_bits(out[name][k]), _bits(host_out[name][k])), name
    for name, worst in mx.items():
        bound = R.device_bound("random", name)
        if name in R.STATED:
            assert worst < bound, (name, worst, bound)
        else:
            assert worst <= bound, (name, worst, bound)
    assert mx["cexp"] <= mx["cexp_tab"] + 0.25


def test_math_edges(dev):
    """(b) rint ties and negative table indices, denormal results, the clamps, the limits of the fast phase range, NaN and
    infinities; unit max(|ref| 2^-53, 2^-1074) (complex forms: 2^-53 e^x, at least 2^-1074).  Bound: host maximum + 1 --
    exp_neg 0.99 -> 1.99, exp_neg_tab 1.27 -> 2.27, sincos_cw 0.96 -> 1.96, cexp_step and <true> 2.13 -> 3.13,
    cexp_step_tab and <true> 1.44 -> 2.44.  NaN in gives NaN out (a reference NaN demands a NaN).  x = -inf belongs to the
    |x| >~ 1e52 of the comment in exp_neg_tab: 0 or NaN / inf, never a finite value other than 0."""
    mx, minf, out = R.measure_edges("device")
    _report("edges", mx)
    for name, worst in mx.items():
        assert worst <= R.device_bound("edges", name), (name, worst)
    assert all(minf.values()), minf


@pytest.mark.parametrize("name", R.COMPLEX_FORMS)
def test_math_mixed_waves(dev, name):
    """(c) One lane beyond the fast range (5e6 / 2e5 rad) or with a NaN phase switches the WAVE to the per-lane form: the 63
    fast lanes return the bits of the all-fast launch (the claim of the comment above cexp_step), the slow lane is held to
    mpmath: host maximum + 1 -- cexp_step 0.68 -> 1.68, <true> 1.17 -> 2.17, cexp_step_tab 0.80 -> 1.80, <true> 1.12 -> 2.12."""
    re0, im0 = R.run_mixed(name, None, None, "device")
    worst = 0.0
    for lane in R.MIXED_LANES:
        fast = np.arange(64) != lane
        re, im = R.run_mixed(name, lane, "slow", "device")
        assert np.array_equal(_bits(re)[fast], _bits(re0)[fast]) and np.array_equal(_bits(im)[fast], _bits(im0)[fast]), lane
        worst = max(worst, R.cerr_units(re[lane:lane + 1], im[lane:lane + 1], R.slow_lane_ref(name, lane)).max())
        re, im = R.run_mixed(name, lane, "nan", "device")
        assert np.array_equal(_bits(re)[fast], _bits(re0)[fast]) and np.array_equal(_bits(im)[fast], _bits(im0)[fast]), lane
        assert np.isnan(re[lane]) and np.isnan(im[lane])
    print("device slow lane %s: %.3f" % (name, worst))
    assert worst <= R.device_bound("slow", name), worst


def _grp_columns(G, moves_only):
    cols = []
    for key, width in (("partner", 1), ("bc_c", G), ("bc_ci", G), ("bc_u", G), ("bc_iu", G), ("bcast", 1), ("bcast_i", 1),
                       ("peek", 4 * G), ("peekk2", G), ("peek2", 2 * G), ("wave_all", 1)) + \
            (() if moves_only else (("sum", 1), ("max", 1))):
        cols += list(range(R.GO[key], R.GO[key] + width))
    return np.array(sorted(cols))


@pytest.mark.parametrize("threads", [64, 256])
@pytest.mark.parametrize("G", [2, 4, 8, 16])
def test_lane_groups(dev, G, threads):
    """(d) Every word the kernel writes, bit for bit against numpy indexing: sum and max in the partner order of grp_emu.h
    and identical in every lane of a group; the broadcasts and the three LDS exchanges are exact moves (a second launch
    carries -0.0, denormals, infinities and NaNs with payloads); wave_all with no and with one false lane.  512 lanes: at
    256 threads per block waves 1-3 use their own 64 exchange slots."""
    n = 512
    rng = np.random.default_rng(100 * G + threads)
    jsrc = np.repeat(rng.integers(0, G, n // G), G)
    for special in (False, True):
        v, iv = R.grp_inputs(n, 7 * G + threads + special, special)
        flag = np.ones(n, dtype=np.int32)
        for wave, lane in ((1, 0), (3, 31), (6, 63)):                    # waves 0, 2, 4, 5, 7: all true
            flag[64 * wave + lane] = 0
        got = R.run_grp(G, v, iv, jsrc, flag, threads)
        want = R.grp_expected(G, v, iv, jsrc, flag)
        cols = _grp_columns(G, special)
        bad = np.argwhere(got[:, cols] != want[:, cols])
        assert bad.size == 0, "G=%d: lane %d word %d" % (G, bad[0][0], cols[bad[0][1]])
        assert sorted(set(got[:, R.GO["wave_all"]].reshape(-1, 64)[:, 0])) == [0, 1]
        if not special:
            for key in ("sum", "max"):
                col = got[:, R.GO[key]].reshape(-1, G)
                assert (col == col[:, :1]).all(), key
            written = np.zeros(R.GRP_OUT, dtype=bool)
            written[_grp_columns(G, False)] = True
            assert (got[:, ~written] == 0).all()                          # slots of lanes J >= G stay as the launcher zeroed them


def _row_case(P, seed):
    x = R.row_inputs(64, seed)
    rng = np.random.default_rng(seed + 1)
    e, y = float(-rng.uniform(0.5, 2.0)), float(rng.uniform(-2.0, 2.0))      # negative e: the block takes |e|
    return x, e, y


@pytest.mark.parametrize("P", [2, 3, 4, 5, 6, 7])
def test_row_blocks(dev, P):
    """(e) RowAsm<P> in a wave of four independent rows.  colmix and gain_nt: the fma sequence of grp_emu.h::row_colmix / one
    fma, bit for bit.  lazy_front (w, var, k) and innov_t2: the formula of the header's comment in mpmath, within
    (P + 3) 2^-53 sum |terms| (each rounding is at most half an ulp of a partial sum, which the sum of the magnitudes bounds;
    var's terms are taken down to the products S_i@j ht@i ht@j because t@j carries the roundings of w@j).  Lanes P..15 and
    the other rows do not reach a row's outputs: changed there, and with the rows rotated, not a bit moves."""
    x, e, y = _row_case(P, 1000 + P)
    out = R.run_row(P, x, e, y)
    tol = (P + 3) * R.U53
    for row in range(4):
        xr, o = x[16 * row:16 * row + 16], out[16 * row:16 * row + 16]
        c, s = xr[:, R.RI["c"]], xr[:, R.RI["s"]]
        mm = R.row_colmix_ref(P, c, s, xr[:, R.RI["D"]:R.RI["D"] + P])
        assert np.array_equal(_bits(o[:P, R.RO["mm"]:R.RO["mm"] + P]), _bits(mm[:P])), "colmix"
        sg = R.row_gain_ref(P, xr[:, R.RI["S"]:R.RI["S"] + P], xr[:, R.RI["k"]], xr[:, R.RI["nt"]])
        assert np.array_equal(_bits(o[:P, R.RO["S"]:R.RO["S"] + P]), _bits(sg[:P])), "gain_nt"
        front = R.row_front_ref(P, xr, e)
        front["innov"] = R.row_innov_ref(P, xr, y)
        for key, (val, mag) in front.items():
            for r in range(P):
                err = abs(R.MP.mpf(float(o[r, R.RO[key]])) - val[r])
                assert err <= tol * mag[r], (key, row, r, float(err / (R.U53 * mag[r])))
    live = np.zeros((64, R.ROW_OUT), dtype=bool)
    live[(np.arange(64) % 16) < P] = True
    live[:, R.RO["mm"] + P:R.RO["mm"] + 7] = False
    live[:, R.RO["S"] + P:R.RO["S"] + 7] = False
    # other finite values in lanes P..15 of every row, for every per-lane input
    x2 = x.copy()
    dead = (np.arange(64) % 16) >= P
    x2[dead] = R.row_inputs(64, 2000 + P)[dead]
    out2 = R.run_row(P, x2, e, y)
    assert np.array_equal(_bits(out2)[live], _bits(out)[live])
    # rows rotated inside the wave: every row meets three other neighbours, its outputs travel with it
    rot = np.roll(np.arange(64), 16)
    out3 = R.run_row(P, x[rot], e, y)
    assert np.array_equal(_bits(out3)[live], _bits(out[rot])[live])
    # a row alone among rows of different data
    x4 = R.row_inputs(64, 3000 + P)
    x4[16:32] = x[16:32]
    out4 = R.run_row(P, x4, e, y, threads=64)
    assert np.array_equal(_bits(out4[16:32])[live[16:32]], _bits(out[16:32])[live[16:32]])


def test_philox_known_answers(dev):
    """(f) philox4x32_10 on the device: the three Random123 known-answer vectors, in every lane position of a block."""
    words = np.array([w for w, _ in R.PHILOX_KAT] * 86, dtype=np.uint32)[:256]
    want = np.array([o for _, o in R.PHILOX_KAT] * 86, dtype=np.uint32)[:256]
    got, u = R.run_philox(words)
    assert np.array_equal(got, want)
    assert np.array_equal(_bits(u), _bits([R.u01_ref(o[0], o[1]) for o in want]))
    assert ((u > 0.0) & (u < 1.0)).all()


def test_rng_draws(dev):
    """(f) 4096 keys, every lane its own (seed, chain, iter, purpose, idx), with iter = 0, 2^32 - 1, 2^32, 2^40 + 5, chain = 0,
    2^32 - 1, seeds with high bits set, idx = 0, 6, 13, 2^23 - 1 and all four purposes.  rng_uniform: the Python Philox bit for
    bit (integer operations and one exact conversion).  rng_normal: |dz| <= 16 2^-53 sqrt(-2 ln u1) against mpmath on the
    same words (the rounding of 2 pi u2 is at most 3.2 units, log, sqrt and cos a few ulp each).  rng_student_t8: that bound
    over sqrt(chi2 / 8), plus 8 2^-53 |t| for the denominator."""
    key, it = R.rng_keys()
    ref = R.rng_refs()
    got = R.run_rng(key, it)
    assert np.array_equal(_bits(got[:, 0]), _bits(ref["uniform"]))
    assert ((got[:, 0] > 0.0) & (got[:, 0] < 1.0)).all()
    ez = R.err_units(got[:, 1], ref["normal"])
    et = R.err_units(got[:, 2], ref["t8"])
    print("rng_normal: largest |dz| / bound %.3f; rng_student_t8: %.3f" % ((ez / ref["normal_bound"]).max(), (et / ref["t8_bound"]).max()))
    assert (ez <= ref["normal_bound"]).all()
    assert (et <= ref["t8_bound"]).all()
