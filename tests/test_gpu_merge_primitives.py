"""The three pieces of device code under the two-sided kernels that the suite reached only end to end, each on its own
(tests/devprim/devprim.hip, references in tests/devprim_ref.py):

  pipew_merge<P>          against the closed form N = I - Da Db in mpmath at 120 digits, on synthetic (X, Y, a, beta) of every rank
                          and on the outputs of real half filters; and the properties that hold exactly: a row pair's bits do not
                          depend on the other evaluation of its wave, on its slot, on the data lanes or on the unread triangle of Da,
                          and not on a rescaling of the coordinates by powers of two.
  WinAsm<P>::init/chunk   init bit for bit; chunk against the mpmath elimination within a running first-order error bound; neutral
                          slots, independence of the rows, the caller's EXEC handed back.
  rcp / rsq, recip(), rsqrt_pos()   the accuracies DESIGN.md section 4 builds on.

The constant in front of the merge's error unit U = 2^-53 kappa S is not derivable; it is the float64 restatement's
(two_sided.merge_chol) maximum over the same arrays, devprim_ref.HOST_MAX["merge"][P], which tests/test_devprim_cpu.py holds the
restatement to; the device may use twice that.  After a launcher has returned a HIP error nothing more is launched."""
import numpy as np
import pytest

import devprim_ref as R
from helpers import record_allowance

pytestmark = pytest.mark.gpu

ORDERS = R.MERGE_ORDERS


@pytest.fixture(scope="module")
def dev():
    L = R.device()
    assert L.devprim_device_count() >= 1
    return L


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _pct(fraction):
    """Percent of an allowance, for helpers.record_allowance (integers)."""
    return int(min(np.ceil(100.0 * fraction), 10 ** 6)) if fraction == fraction else 10 ** 6


def _run_evals(P, evs):
    """Evaluations two per wave -> (values [n], words [n, 32, 2] uint64)."""
    evs = list(evs)
    pad = evs + [None] * (len(evs) & 1)
    x = np.concatenate([R.merge_pack(P, pad[i:i + 2]) for i in range(0, len(pad), 2)])
    out = R.run_merge(P, x)
    vals, words = [], []
    for i in range(len(evs)):
        v, w = R.merge_result(P, out, i // 2, i & 1)
        vals.append(v)
        words.append(w)
    return np.array(vals), np.array(words)


def _pow2_scaled(ev, k):
    """X -> D X D, Y -> D^-1 Y D^-1, a -> D a, beta -> D^-1 beta with D = diag(2^k); None where a scaled entry would leave the
    normal range (the scaling is then not exact)."""
    Da, a, Db, beta = ev
    kk = k[:, None] + k[None, :]
    out = (np.ldexp(Da, kk), np.ldexp(a, k), np.ldexp(Db, -kk), np.ldexp(beta, -k))
    back = (np.ldexp(out[0], -kk), np.ldexp(out[1], -k), np.ldexp(out[2], kk), np.ldexp(out[3], k))
    tiny = 2.0 ** -1000
    for o, b, src in zip(out, back, ev):
        if not (np.array_equal(b, src) and np.isfinite(o).all() and np.all((o == 0) | (np.abs(o) > tiny))):
            return None
    return out


def _exact_bases(P):
    """(name, evaluation): one synthetic evaluation of every rank at lambda_max = 0.99, the tie and rank-cut shapes, and the first
    real half-filter outputs of this order."""
    cases = R.merge_cases(P)
    seen, out = set(), []
    for i, (fam, ev) in enumerate(cases):
        key = fam
        if fam.startswith("rank"):
            if (i // R.MERGE_DRAWS) % len(R.MERGE_LAMS) != 1:
                continue
        if key not in seen:
            seen.add(key)
            out.append((fam, ev))
    if P in R.REAL_P:
        out += [("real%d" % i, ev) for i, (_, ev) in enumerate(R.real_cases(P)[:6])]
    return out


@pytest.mark.parametrize("P", ORDERS)
def test_merge_exact_properties(dev, P):
    """No tolerance.  The same launch twice: the same bits.  An evaluation's 32 lanes (per-lane total and the row pair's sum) keep
    their bits when the other evaluation of the wave is one of another rank, all zero, all NaN, or one with lambda_max(X Y) = 1.5
    (which itself gives NaN, and only it); when the evaluation sits in slot 1 instead of slot 0; when the data lanes carry NaN; when
    the elements of Da above the diagonal are replaced; and under X -> D X D, Y -> D^-1 Y D^-1, a -> D a, beta -> D^-1 beta with
    D = diag(2^k), k odd and even in [-300, 300] (the claim of the comment above the equilibration).  Every lane but the backward
    row's virtual lanes contributes exactly 0.0, and the pair's sum is the same in its 32 lanes."""
    ND = 16 - P
    rng = np.random.default_rng(7700 + P)
    bases = _exact_bases(P)
    cases = R.merge_cases(P)
    nan_ev = tuple(np.full(np.shape(v), np.nan) for v in cases[0][1])
    Da5, a5, Db5, b5 = cases[-1][1]
    lam = R._lam_max(-R.lower_sym(Da5), -Db5)
    over = (Da5, a5, Db5 * (1.5 / lam), b5)                       # lambda_max(X Y) = 1.5
    blocks, plan = [], []
    for bi, (name, ev) in enumerate(bases):
        other = bases[(bi + 1) % len(bases)][1]
        Da = np.array(ev[0])
        up = Da.copy()
        up[np.triu_indices(P, 1)] = rng.standard_normal(P * (P - 1) // 2) * 1e3
        k = rng.integers(-300, 301, P)
        k[0], k[1] = k[0] | 1, k[1] & ~1
        scaled = _pow2_scaled((R.lower_sym(Da), ev[1], ev[2], ev[3]), k)
        variants = [("again", (ev, other), 0, 0.0), ("other rank", (ev, bases[(bi + 2) % len(bases)][1]), 0, 0.0),
                    ("zeros", (ev, None), 0, 0.0), ("NaN neighbour", (ev, nan_ev), 0, 0.0), ("lambda 1.5 neighbour", (ev, over), 0, 0.0),
                    ("slot 1", (other, ev), 1, 0.0), ("slot 1, NaN neighbour", (nan_ev, ev), 1, 0.0),
                    ("NaN data lanes", (ev, other), 0, np.nan), ("upper triangle", ((up, ev[1], ev[2], ev[3]), other), 0, 0.0)]
        if scaled is not None:
            variants.append(("powers of two", (scaled, other), 0, 0.0))
        plan.append((name, len(blocks), variants))
        blocks.append(R.merge_pack(P, (ev, other)))
        for _, slots, _, fill in variants:
            blocks.append(R.merge_pack(P, slots, data_fill=fill))
    x = np.concatenate(blocks)
    out = R.run_merge(P, x)
    assert np.array_equal(_bits(out), _bits(R.run_merge(P, x))), "two launches differ"
    nscaled = 0
    for name, b0, variants in plan:
        val, ref = R.merge_result(P, out, b0, 0)
        assert np.isfinite(val), name
        assert (ref[:, 1] == ref[0, 1]).all(), (name, "the pair's sum differs between its lanes")
        tot = out[b0, :32, 0]
        contributes = np.zeros(32, dtype=bool)
        contributes[16 + ND:] = True
        assert np.all(tot[~contributes] == 0.0), (name, "a lane other than the backward row's virtual lanes contributes")
        with np.errstate(all="ignore"):
            want = R.butterfly(tot[16:], 16, np.add)[0] + R.butterfly(tot[:16], 16, np.add)[0]
        assert _bits(val) == _bits(want), (name, "the pair's sum is not the butterfly sum of the lanes' totals")
        for k_, (what, _, slot, _) in enumerate(variants):
            _, got = R.merge_result(P, out, b0 + 1 + k_, slot)
            assert np.array_equal(got, ref), (name, what)
            nscaled += what == "powers of two"
            if "lambda" in what or (what == "NaN neighbour"):
                assert np.isnan(R.merge_result(P, out, b0 + 1 + k_, 1)[0]), (name, what)
    assert nscaled >= P                                          # (every synthetic base takes the scaling)


@pytest.mark.parametrize("P", ORDERS)
def test_merge_synthetic_families(dev, P):
    """X = B B^T of every rank 0 .. P, Y random with lambda_max(X Y) = 0.3, 0.99, 1 - 1e-6, 8 draws each; a unit-diagonal X and
    X = 3 I (every pivot a tie); a pivot at 4e-14 (taken) and at 4e-16 (either decision passes: the allowance is widened by
    |truth(delta) - truth(0)|); a diagonal entry of -1e-17.  |device - mpmath| <= 2 HOST_MAX["merge"][P] U with U = 2^-53 kappa S,
    kappa = 1 / (1 - lambda_max), S the sum of the terms' magnitudes; rank 0 has the derived bar (P + 2) 2^-53 S."""
    cases = R.merge_cases(P)
    vals, _ = _run_evals(P, [ev for _, ev in cases])
    factor = 2.0 * R.HOST_MAX["merge"][P]
    worst, worst0, err = R.merge_measure(P, vals)
    allow = R.merge_allowance(P, factor)
    print("merge, P = %d, %d evaluations: largest |device - truth| / U %.3f of %.2f allowed (%.0f %%); rank 0: %.3f of its derived bar"
          % (P, len(cases), worst, factor, 100.0 * worst / factor, worst0))
    record_allowance("merge-unit", "P=%d: percent of 2 x host maximum x U used" % P, _pct(worst / factor), 100,
                     population=len(cases), worst_device=worst, worst_oracle=R.HOST_MAX["merge"][P])
    bad = [(cases[i][0], err[i], allow[i]) for i in range(len(cases)) if not err[i] <= allow[i]]
    assert not bad, bad[:5]


@pytest.mark.parametrize("P", R.REAL_P)
def test_merge_real_half_filters(dev, P):
    """(Da, a, Db, beta) of two_sided.half_filter on prior-like draws, n = 6, 20, 41, 120 (P = 3: the state with two real roots
    6e-4 apart).  X is indefinite at rounding level there and the merge drops those directions on purpose, so the closed form has no
    derivable bar; the measure is the distance relative to the whole log-likelihood |l_a + l_b + merge|, the yardstick the float64
    restatement's maximum in that measure, HOST_MAX["merge_real"][P]: the device may be at twice it, and at least 16 2^-53."""
    cases = R.real_cases(P)
    assert len(cases) >= 1
    vals, _ = _run_evals(P, [ev for _, ev in cases])
    worst = R.real_measure(P, vals)
    allowed = max(2.0 * R.HOST_MAX["merge_real"][P], R.REAL_FLOOR)
    print("merge on real half filters, P = %d, %d evaluations: largest |device - truth| / |log-likelihood| %.3g of %.3g allowed (%.0f %%)"
          % (P, len(cases), worst, allowed, 100.0 * worst / allowed))
    record_allowance("merge-real", "P=%d: percent of max(2 x host maximum, 16 x 2^-53) used" % P, _pct(worst / allowed), 100,
                     population=len(cases), worst_device=worst, worst_oracle=R.HOST_MAX["merge_real"][P])
    assert worst <= allowed


def _rows_rotated(x):
    return x[np.roll(np.arange(64), 16)]


@pytest.mark.parametrize("P", ORDERS)
def test_win_init(dev, P):
    """WinAsm<P>::init, four independent rows: the FMA chain in the generator's order, bit for bit; the data lanes' kk and nuF and
    the other rows do not reach a row's outputs."""
    ND = 16 - P
    x = R.win_init_inputs(P, 300 + P)
    out = R.run_win_init(P, x)
    for row in range(4):
        want = R.win_init_ref(P, x[16 * row:16 * row + 16])
        assert np.array_equal(_bits(out[16 * row:16 * row + 16]), _bits(want)), row
    x2 = x.copy()
    data = (np.arange(64) % 16) < ND
    x2[np.ix_(data, np.arange(P + 1, 2 * P + 2))] = R.win_init_inputs(P, 400 + P)[np.ix_(data, np.arange(P + 1, 2 * P + 2))]
    assert np.array_equal(_bits(R.run_win_init(P, x2)), _bits(out))
    assert np.array_equal(_bits(R.run_win_init(P, _rows_rotated(x))), _bits(_rows_rotated(out)))
    x4 = R.win_init_inputs(P, 500 + P)
    x4[32:48] = x[32:48]
    assert np.array_equal(_bits(R.run_win_init(P, x4)[32:48]), _bits(out[32:48]))


@pytest.mark.parametrize("P", ORDERS)
def test_win_chunk(dev, P):
    """WinAsm<P>::chunk, four independent rows, two kinds of chunk (measurement noise of the size of the signal, with a gain
    offset; noise 1e-3 of it, so that the pivots cancel): each data lane's final variance and innovation (mA / nuA for an even
    lane, mB / nuB for an odd one), the virtual lanes' kk (the columns of S) and their nu (in B where ND is odd) against the mpmath
    elimination within the running first-order bound of devprim_ref.win_chunk_truth (eps_t = 2^-48).  A row's outputs do not depend
    on the other rows."""
    worst = 0.0
    for seed, noise, gain in ((600 + P, 1.0, 0.5), (700 + P, 1e-3, 0.0)):
        x = R.win_chunk_inputs(P, seed, noise, gain)
        out, marker = R.run_win_chunk(P, x)
        assert (marker == 1).all()
        for row in range(4):
            val, err = R.win_chunk_truth(P, x[16 * row:16 * row + 16])
            w = R.win_chunk_worst(P, out[16 * row:16 * row + 16], val, err)
            worst = max(worst, w)
            assert w <= 1.0, (seed, row, w)
        out3, _ = R.run_win_chunk(P, _rows_rotated(x))
        assert np.array_equal(_bits(out3), _bits(_rows_rotated(out)))
        x4 = R.win_chunk_inputs(P, seed + 50, noise, gain)
        x4[16:32] = x[16:32]
        out4, _ = R.run_win_chunk(P, x4)
        assert np.array_equal(_bits(out4[16:32]), _bits(out[16:32]))
    print("WinAsm<%d>::chunk: largest |device - truth| / running bound %.3f" % (P, worst))
    record_allowance("win-chunk-bound", "P=%d: percent of the running error bound used" % P, _pct(worst), 100,
                     worst_device=worst)


@pytest.mark.parametrize("P", ORDERS)
def test_win_chunk_neutral_slots(dev, P):
    """A chunk of neutral slots (hh = kk = 0, m = 1, nu = 0) leaves the virtual lanes as they were, bit for bit: S, and the
    variance and -z~ in both of their registers."""
    ND = 16 - P
    x = R.win_neutral_inputs(P, 800 + P)
    out, _ = R.run_win_chunk(P, x)
    virt = (np.arange(64) % 16) >= ND
    assert np.array_equal(_bits(out[virt, :P]), _bits(x[virt, :P]))
    for c in (P, P + 1):
        assert np.array_equal(_bits(out[virt, c]), _bits(x[virt, 2 * P]))
        assert np.array_equal(_bits(out[virt, c + 2]), _bits(x[virt, 2 * P + 1]))


@pytest.mark.parametrize("P", ORDERS)
def test_win_chunk_hands_back_the_callers_exec(dev, P):
    """The call under `if (row active)` with two of the four rows inactive: behind the call the marker and the outputs are stored
    by the active lanes and by no other (the block narrows EXEC per pivot and has to restore the caller's mask, not all ones), and
    the active rows' outputs are those of the full-wave call."""
    x = R.win_chunk_inputs(P, 900 + P, 1.0, 0.5)
    full, _ = R.run_win_chunk(P, x)
    for rows in (0b0101, 0b1010, 0b1000):
        out, marker = R.run_win_chunk(P, x, rows=rows)
        active = ((rows >> (np.arange(64) // 16)) & 1).astype(bool)
        assert np.array_equal(marker, active.astype(np.int32)), bin(rows)
        assert np.array_equal(_bits(out[active]), _bits(full[active])), bin(rows)
        assert (out[~active] == R.WIN_FILL).all(), bin(rows)


def test_reciprocals(dev):
    """v_rcp_f64 / v_rsq_f64 over every binade with a normal result and a mantissa sweep, 20 000 values each: relative error
    <= 2^-24 (the project's figure, from another sample, is 2^-24.4).  recip() and rsqrt_pos() on the same arguments against
    mpmath: a stated 2 units of 2^-53 |value| (the host build of recip() divides, so there is no host maximum to start from)."""
    ld = np.longdouble
    x = R.binade_sweep("rcp")
    r, _ = R.run_math("rcp_raw", x)
    e_rcp = float(np.max(np.abs(r.astype(ld) * x.astype(ld) - 1)))
    x2 = R.binade_sweep("rsq")
    r2, _ = R.run_math("rsq_raw", x2)
    # r^2 x = (1 + e)^2: e = (r^2 x - 1) / 2 to first order (the second order is 2^-49)
    e_rsq = float(np.max(np.abs(r2.astype(ld) * r2.astype(ld) * x2.astype(ld) - 1))) / 2
    print("raw v_rcp_f64: largest relative error 2^%.2f; raw v_rsq_f64: 2^%.2f" % (np.log2(e_rcp), np.log2(e_rsq)))
    assert e_rcp <= R.RCP_RAW_BOUND and e_rsq <= R.RCP_RAW_BOUND
    u_rcp = R.err_units(R.run_math("recip", x)[0], R.recip_refs("rcp")).max()
    u_rsq = R.err_units(R.run_math("rsqrt_pos", x2)[0], R.recip_refs("rsq")).max()
    print("recip(): %.3f units of 2^-53; rsqrt_pos(): %.3f" % (u_rcp, u_rsq))
    record_allowance("recip-units", "percent of the 2 units used by recip(), rsqrt_pos()", _pct(max(u_rcp, u_rsq) / R.RECIP_UNITS),
                     100, population=x.size + x2.size, worst_device=max(u_rcp, u_rsq))
    assert u_rcp <= R.RECIP_UNITS and u_rsq <= R.RECIP_UNITS
