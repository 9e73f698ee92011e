"""Builds and loads the device-primitive harness (tests/devprim/devprim.hip) and the host build of carma_math.h
(tests/devprim/hostmath.cpp); the argument arrays of the primitive tests; their references, mpmath at 50 digits and numpy
restatements of grp_device.h / carma_row_asm.h / carma_rng.h; for the two-sided merge (carma_pipew.h pipew_merge) the closed form
in mpmath at 120 digits, for the window blocks (carma_win_asm.h) the elimination of tools/gen_win_asm.py's docstring in mpmath
with a running error bound.  Test code only."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "carma_pack_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
DEV_SRC = os.path.join(HERE, "devprim", "devprim.hip")
DEV_SO = os.path.join(HERE, "devprim", "libdevprim.so")
HOST_SRC = os.path.join(HERE, "devprim", "hostmath.cpp")
HOST_SO = os.path.join(HERE, "devprim", "libhostmath.so")
DEV_HEADERS = ("grp_device.h", "carma_types.h", "carma_row_asm.h", "carma_math.h", "carma_math_tab.h", "carma_rng.h", "carma_core.h",
               "carma_pipew.h", "carma_pipe3l.h", "carma_win_asm.h")

MP = mp.mp.clone()
MP.dps = 50
U53 = 2.0 ** -53
TINY = 5e-324                                                # 2^-1074

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_up = C.POINTER(C.c_uint32)
_qp = C.POINTER(C.c_uint64)


def _stale(so, deps):
    return not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps)


def build_device(force=False, out=None):
    """hipcc with the flags of build.sh -> tests/devprim/libdevprim.so; rebuilt when the source or a header is newer."""
    so = out or DEV_SO
    deps = [DEV_SRC] + [os.path.join(CSRC, h) for h in DEV_HEADERS]
    if force or _stale(so, deps):
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-shared", "-I", CSRC, "-o", so, DEV_SRC],
                       check=True, timeout=300)
    return so


@functools.lru_cache(None)
def device():
    # one process, ONE HIP runtime: the product's loader decides which copy the process maps (carma_pack_amd/_lib.py,
    # _share_with_torch); loading this harness first would map the system's and leave the product without devices
    import carma_pack_amd._lib  # noqa: F401
    L = C.CDLL(build_device())
    L.devprim_math.argtypes = [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]
    L.devprim_grp.argtypes = [C.c_int, C.c_int, C.c_int, _dp, _ip, _ip, _ip, _qp]
    L.devprim_row.argtypes = [C.c_int, C.c_int, C.c_int, _dp, C.c_double, C.c_double, _dp]
    L.devprim_philox.argtypes = [C.c_int, C.c_int, _up, _up, _dp]
    L.devprim_rng.argtypes = [C.c_int, C.c_int, _up, _qp, _dp]
    L.devprim_merge.argtypes = [C.c_int, C.c_int, _dp, _dp]
    L.devprim_win_init.argtypes = [C.c_int, C.c_int, _dp, _dp]
    L.devprim_win_chunk.argtypes = [C.c_int, C.c_int, _dp, _dp, _ip]
    L.devprim_win_chunk_masked.argtypes = [C.c_int, C.c_int, C.c_int, _dp, _dp, _ip]
    return L


@functools.lru_cache(None)
def host():
    deps = [HOST_SRC, os.path.join(CSRC, "carma_math.h"), os.path.join(CSRC, "carma_math_tab.h")]
    if _stale(HOST_SO, deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-mfma", "-ffp-contract=off", "-I", CSRC, "-o", HOST_SO,
                        HOST_SRC], check=True, timeout=300)
    L = C.CDLL(HOST_SO)
    L.hostmath.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]
    return L


# ---- a HIP error ends the module: nothing more is launched after a launcher returned non-zero -------------------------
HIP_ERROR = [None]


def launch(fn, *args):
    import pytest
    if HIP_ERROR[0] is not None:
        pytest.fail("harness reported HIP error %d earlier" % HIP_ERROR[0])
    rc = fn(*args)
    if rc != 0:
        HIP_ERROR[0] = int(rc)
        pytest.fail("harness reported HIP error %d" % rc)


def _f64(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def _ptr(a, t=_dp):
    return a.ctypes.data_as(t)


FN = dict(exp_neg=0, exp_neg_tab=1, sincos_cw=2, cexp=3, cexp_tab=4, cexp_exact=5, cexp_tab_exact=6,
          recip=7, rsqrt_pos=8, rcp_raw=9, rsq_raw=10)         # (7 .. 10: device only -- on the host recip() is a division)
COMPLEX_FORMS = ("cexp", "cexp_tab", "cexp_exact", "cexp_tab_exact")


def _pad(x, n, fill):
    out = np.full(n, fill, dtype=np.float64)
    out[:x.size] = x
    return out


def run_math(name, a, b=None, dt=None, dt_lo=None, threads=256, on="device"):
    """One primitive per lane over the arrays; the launch is padded to full blocks with harmless arguments."""
    a = _f64(a)
    n = a.size
    b = np.zeros(n) if b is None else _f64(b)
    dt = np.ones(n) if dt is None else _f64(dt)
    dt_lo = np.zeros(n) if dt_lo is None else _f64(dt_lo)
    m = -(-n // threads) * threads
    A, B, D, L = _pad(a, m, -0.5), _pad(b, m, 0.25), _pad(dt, m, 1.0), _pad(dt_lo, m, 0.0)
    o0, o1 = np.full(m, -7.0), np.full(m, -7.0)
    if on == "device":
        launch(device().devprim_math, FN[name], m, threads, _ptr(A), _ptr(B), _ptr(D), _ptr(L), _ptr(o0), _ptr(o1))
    else:
        assert host().hostmath(FN[name], m, _ptr(A), _ptr(B), _ptr(D), _ptr(L), _ptr(o0), _ptr(o1)) == 0
    return o0[:n], o1[:n]


# ---- (a) random arguments: the distribution of tests/tools/proto/table_math_accuracy.cpp -------------------------------
@functools.lru_cache(None)
def random_triples(n=20000, seed=20240611):
    """a = -10^U(-6,2), b = +-10^U(-6,3), dt = 10^U(-3,3), |b dt| < 9e4, a dt >= -700; dt_lo of relative size <= 2^-53."""
    rng = np.random.default_rng(seed)
    a, b, dt = np.empty(0), np.empty(0), np.empty(0)
    while a.size < n:
        ca = -10.0 ** rng.uniform(-6, 2, n)
        cb = np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-6, 3, n)
        cd = 10.0 ** rng.uniform(-3, 3, n)
        ok = (np.abs(cb * cd) < 9.0e4) & ~(ca * cd < -700.0)
        a, b, dt = np.r_[a, ca[ok]], np.r_[b, cb[ok]], np.r_[dt, cd[ok]]
    a, b, dt = a[:n].copy(), b[:n].copy(), dt[:n].copy()
    dt_lo = dt * rng.uniform(-1.0, 1.0, n) * U53
    for x in (a, b, dt, dt_lo):
        x.setflags(write=False)
    return a, b, dt, dt_lo


@functools.lru_cache(None)
def big_phase_triples(hi, n=4000, seed=77):
    """The second EXACT set: |b dt| log-uniform in [1e3, hi)."""
    rng = np.random.default_rng(seed + int(hi))
    a, b, dt = np.empty(0), np.empty(0), np.empty(0)
    while a.size < n:
        ca = -10.0 ** rng.uniform(-6, 2, n)
        cd = 10.0 ** rng.uniform(-3, 3, n)
        ph = np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(3.0, np.log10(hi), n)
        cb = ph / cd
        ok = (np.abs(cb * cd) >= 1.0e3) & (np.abs(cb * cd) < hi) & ~(ca * cd < -700.0)
        a, b, dt = np.r_[a, ca[ok]], np.r_[b, cb[ok]], np.r_[dt, cd[ok]]
    a, b, dt = a[:n].copy(), b[:n].copy(), dt[:n].copy()
    dt_lo = dt * rng.uniform(-1.0, 1.0, n) * U53
    for x in (a, b, dt, dt_lo):
        x.setflags(write=False)
    return a, b, dt, dt_lo


# ---- references as (hi, lo) pairs of doubles: ref = hi + lo to ~32 digits ---------------------------------------------
def _split(v):
    """mpf -> (hi, lo); NaN / inf pass through with lo = 0."""
    if not MP.isfinite(v):
        return float(v), 0.0
    hi = float(v)
    return hi, float(v - MP.mpf(hi))


class Ref(object):
    """hi + lo is the exact value; unit the error unit of the entry."""

    def __init__(self, n):
        self.hi, self.lo, self.unit = np.empty(n), np.empty(n), np.empty(n)

    def put(self, i, v, unit):
        self.hi[i], self.lo[i] = _split(v)
        self.unit[i] = max(float(unit), TINY) if MP.isfinite(unit) else np.nan
        return self

    def freeze(self):
        for x in (self.hi, self.lo, self.unit):
            x.setflags(write=False)
        return self

    def __getitem__(self, idx):
        r = Ref(0)
        r.hi, r.lo, r.unit = self.hi[idx], self.lo[idx], self.unit[idx]
        return r


def _mp(x):
    x = float(x)
    if x != x:
        return MP.nan
    return MP.mpf(x)


def _mp_exp(x):
    if x == MP.ninf:
        return MP.mpf(0)
    return MP.exp(x)


def _mp_sincos(x):
    if not MP.isfinite(x):
        return MP.nan, MP.nan
    return MP.sin(x), MP.cos(x)


def _ulp(v):
    """1 ulp of the reference value (2^-1074 in the denormal range and at 0)."""
    return MP.mpf(float(np.spacing(abs(float(v))))) if MP.isfinite(v) else MP.nan


def ref_real(x):
    """exp(x), sin(x), cos(x) of the doubles x.  Unit of exp: max(|ref| 2^-53, 2^-1074), the unit of
    test_table_math_accuracy (never larger than an ulp); of sin and cos: 1 ulp of the reference value."""
    x = _f64(x)
    e, s, c = Ref(x.size), Ref(x.size), Ref(x.size)
    for i, xi in enumerate(x):
        v = _mp(xi)
        ev = _mp_exp(v)
        sv, cv = _mp_sincos(v)
        e.put(i, ev, abs(ev) * U53)
        s.put(i, sv, _ulp(sv))
        c.put(i, cv, _ulp(cv))
    return e.freeze(), s.freeze(), c.freeze()


def ref_cexp(a, b, dt, dt_lo=None, products="rounded"):
    """exp((a + i b) dt) -> (re, im), unit 2^-53 e^x.  products: "rounded" = at fl(a dt), fl(b dt), the contract of the plain
    forms; "exact" = (a + i b) (dt + dt_lo) with the products exact, the contract of the EXACT forms."""
    a, b, dt = _f64(a), _f64(b), _f64(dt)
    dt_lo = np.zeros(a.size) if dt_lo is None else _f64(dt_lo)
    re, im = Ref(a.size), Ref(a.size)
    for i in range(a.size):
        if products == "rounded":
            with np.errstate(all="ignore"):
                x, ph = _mp(a[i] * dt[i]), _mp(b[i] * dt[i])
        else:
            t = _mp(dt[i]) + _mp(dt_lo[i])
            x, ph = _mp(a[i]) * t, _mp(b[i]) * t
        ev = _mp_exp(x)
        sv, cv = _mp_sincos(ph)
        re.put(i, ev * cv, ev * U53)
        im.put(i, ev * sv, ev * U53)
    return re.freeze(), im.freeze()


def err_units(got, ref):
    """|got - ref| in the entry's unit.  A reference NaN wants NaN (error 0, else inf); a non-finite result where the
    reference is finite is an infinite error."""
    got = _f64(got)
    with np.errstate(all="ignore"):
        e = np.abs((got - ref.hi) - ref.lo) / ref.unit
    want_nan = np.isnan(ref.hi)
    e[want_nan] = np.where(np.isnan(got[want_nan]), 0.0, np.inf)
    e[~want_nan & ~np.isfinite(got)] = np.inf
    return e


def cerr_units(re, im, ref):
    return np.maximum(err_units(re, ref[0]), err_units(im, ref[1]))


@functools.lru_cache(None)
def random_refs():
    """References of set (a), computed once: real forms and plain complex forms at the rounded products, the EXACT forms at
    the exact ones (with dt_lo: cexp_step<true>; without: cexp_step_tab<true>)."""
    a, b, dt, dt_lo = random_triples()
    n = a.size
    e, s, c = Ref(n), Ref(n), Ref(n)
    rnd, xlo, xct = (Ref(n), Ref(n)), (Ref(n), Ref(n)), (Ref(n), Ref(n))
    for i in range(n):
        ev = MP.exp(_mp(a[i] * dt[i]))
        sv, cv = _mp_sincos(_mp(b[i] * dt[i]))
        e.put(i, ev, ev * U53)
        s.put(i, sv, _ulp(sv))
        c.put(i, cv, _ulp(cv))
        rnd[0].put(i, ev * cv, ev * U53)
        rnd[1].put(i, ev * sv, ev * U53)
        for pair, t in ((xlo, _mp(dt[i]) + _mp(dt_lo[i])), (xct, _mp(dt[i]))):
            ev = MP.exp(_mp(a[i]) * t)
            sv, cv = _mp_sincos(_mp(b[i]) * t)
            pair[0].put(i, ev * cv, ev * U53)
            pair[1].put(i, ev * sv, ev * U53)
    fz = lambda pair: (pair[0].freeze(), pair[1].freeze())     # noqa: E731
    return dict(exp=e.freeze(), sin=s.freeze(), cos=c.freeze(), rounded=fz(rnd), exact_lo=fz(xlo), exact=fz(xct))


@functools.lru_cache(None)
def big_phase_refs():
    ta, pa = big_phase_triples(9.0e4), big_phase_triples(1.0e6)
    return dict(tab=ref_cexp(ta[0], ta[1], ta[2], None, "exact"), poly=ref_cexp(pa[0], pa[1], pa[2], pa[3], "exact"))


# ---- (b) edges ------------------------------------------------------------------------------------------------------------
def _either_side(v):
    """The two adjacent doubles with lo <= v <= hi (v an mpf that is no double)."""
    f = float(v)
    if MP.mpf(f) > v:
        return [float(np.nextafter(f, -np.inf)), f]
    return [f, float(np.nextafter(f, np.inf))]


@functools.lru_cache(None)
def exp_edges(positive_large=False):
    x = [0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300]
    ln2 = MP.log(2)
    for k in (1, 3, 31, 33, 1023):
        for sg in (1, -1):
            x += _either_side(sg * k * ln2 / 64) + _either_side(sg * k * ln2 / 2)
    x += [-708.3, -708.5, -740.0, -745.1, -745.2, -746.0, float(-2200 * ln2), -1e5]
    if positive_large:
        x += [700.0, 709.7]
    x += [-np.inf, np.nan]
    x = np.array(x)
    x.setflags(write=False)
    return x


@functools.lru_cache(None)
def phase_edges(form):
    """form: "tab" (cexp_step_tab), "poly" (cexp_step), "sincos" (sincos_cw: the finite ones below 2^20)."""
    x = [0.0]
    for k in (1, 63, 64, 65, 2 ** 20 - 1):
        for sg in (1, -1):
            x += [float(sg * k * MP.pi / 64), float(sg * k * MP.pi / 2)]
    if form == "tab":
        x += [float(np.nextafter(98304.0, 0.0)), 98304.0, float(np.nextafter(98304.0, np.inf))]
    if form in ("poly", "sincos"):
        x += [float(np.nextafter(2.0 ** 20, 0.0))]
    if form == "poly":
        x += [2.0 ** 20, 1e9, 1e15]
    if form != "sincos":
        x += [np.nan, np.inf, -np.inf]
    x = np.array(x)
    if form == "sincos":
        x = x[np.abs(x) < 2.0 ** 20]
    x.setflags(write=False)
    return x


EDGE_A, EDGE_B = -0.5, 0.3         # the other argument of a complex form while one runs through its edges (dt = 1)


@functools.lru_cache(None)
def cexp_edges(form):
    """(a, b, dt) with dt = 1, so the products are exact and one reference serves the plain and the EXACT form."""
    xe, pe = exp_edges(), phase_edges(form)
    a = np.r_[xe, np.full(pe.size, EDGE_A)]
    b = np.r_[np.full(xe.size, EDGE_B), pe]
    for x in (a, b):
        x.setflags(write=False)
    return a, b, np.ones(a.size)


@functools.lru_cache(None)
def edge_refs():
    out = dict(exp=ref_real(exp_edges())[0], exp_pos=ref_real(exp_edges(True))[0])
    _, out["sin"], out["cos"] = ref_real(phase_edges("sincos"))
    for form in ("tab", "poly"):
        a, b, dt = cexp_edges(form)
        out[form] = ref_cexp(a, b, dt)
    return out


def exp_minus_inf_ok(got, x):
    """exp(-inf): 0 is exact; NaN / inf is what the comment in exp_neg_tab documents for |x| >~ 1e52 (the reduction leaves
    inf - inf) and every caller treats as a failed evaluation.  Anything finite and non-zero is wrong."""
    m = np.isneginf(x)
    return np.all((got[m] == 0.0) | ~np.isfinite(got[m]))


# ---- (c) mixed waves -----------------------------------------------------------------------------------------------------
def mixed_wave(form, lane, kind):
    """The first 64 triples of set (a); lane `lane` replaced by a phase beyond the fast range (kind "slow": 5e6 for the
    polynomial form, 2e5 for the table form) or by NaN (kind "nan").  lane None: all fast."""
    a, b, dt, dt_lo = (x[:64].copy() for x in random_triples())
    if lane is not None:
        b[lane] = np.nan if kind == "nan" else (5.0e6 if form == "poly" else 2.0e5) / dt[lane]
    return a, b, dt, dt_lo


# ---- the measurements of (a), (b), (c), shared by the host test (CPU) and the device test (GPU) ----------------------------
# Maximum error of the HOST build of carma_math.h (g++ -O2 -mfma -ffp-contract=off, glibc) on exactly these arrays, in the
# units above, rounded up to two decimals; tests/test_devprim_cpu.py holds the host build to them.
HOST_MAX = {
    "random": dict(exp_neg=1.14, exp_neg_tab=1.74, sincos_cw=1.39, cexp=2.98, cexp_tab=2.98, cexp_exact=3.09, cexp_tab_exact=3.07,
                   big_poly_exact=3.34, big_tab_exact=2.84),
    "edges": dict(exp_neg=0.99, exp_neg_tab=1.27, sincos_cw=0.96, cexp=2.13, cexp_exact=2.13, cexp_tab=1.44, cexp_tab_exact=1.44),
    "slow": dict(cexp=0.68, cexp_exact=1.17, cexp_tab=0.80, cexp_tab_exact=1.12),
    # the float64 restatement of the merge (two_sided.merge_chol) against mpmath on merge_cases(P): largest error in units
    # U = 2^-53 kappa S over every family but rank 0 (derived bar) and the pivot at 4e-16 (widened allowance) ...
    "merge": {2: 15.23, 3: 8.32, 4: 4.38, 5: 4.94, 6: 4.16, 7: 4.70},
    # ... and on real_cases(P): largest error relative to the whole log-likelihood |l_a + l_b + merge|
    "merge_real": {2: 1.75e-15, 3: 6.63e-9, 5: 1.67e-15, 7: 9.9e-16},
}
# What the project states: exp_neg_tab < 2.0 and cexp_step_tab < 3.6 (test_emu_core.py::test_table_math_accuracy), exp_neg and
# sincos_cw < 2 (header of carma_math.h); cexp_step <= cexp_step_tab + 0.25 (the same test's relation read the other way).
STATED = dict(exp_neg=2.0, exp_neg_tab=2.0, sincos_cw=2.0, cexp_tab=3.6, cexp=3.6 + 0.25)


def device_bound(kind, name):
    """The project's number where it states one (random arguments of the plain forms); elsewhere -- the EXACT forms, the
    edges with their denormal-range results, the library slow path -- the host maximum plus one unit: host and device do the
    same FMA sequences and can differ only in ldexp, rint, sin and cos of the two libraries."""
    if kind == "random" and name in STATED:
        return STATED[name]
    return HOST_MAX[kind][name] + 1.0


def measure_random(on):
    """-> ({name: maximum error}, {name: outputs}) of set (a) and of the second EXACT set."""
    a, b, dt, dt_lo = random_triples()
    rr = random_refs()
    out = dict(exp_neg=run_math("exp_neg", a * dt, on=on), exp_neg_tab=run_math("exp_neg_tab", a * dt, on=on),
               sincos_cw=run_math("sincos_cw", b * dt, on=on), cexp=run_math("cexp", a, b, dt, on=on),
               cexp_tab=run_math("cexp_tab", a, b, dt, on=on), cexp_exact=run_math("cexp_exact", a, b, dt, dt_lo, on=on),
               cexp_tab_exact=run_math("cexp_tab_exact", a, b, dt, on=on))
    ta, pa = big_phase_triples(9.0e4), big_phase_triples(1.0e6)
    out["big_tab_exact"] = run_math("cexp_tab_exact", ta[0], ta[1], ta[2], on=on)
    out["big_poly_exact"] = run_math("cexp_exact", pa[0], pa[1], pa[2], pa[3], on=on)
    br = big_phase_refs()
    mx = dict(exp_neg=err_units(out["exp_neg"][0], rr["exp"]).max(), exp_neg_tab=err_units(out["exp_neg_tab"][0], rr["exp"]).max(),
              sincos_cw=max(err_units(out["sincos_cw"][0], rr["sin"]).max(), err_units(out["sincos_cw"][1], rr["cos"]).max()),
              cexp=cerr_units(*out["cexp"], rr["rounded"]).max(), cexp_tab=cerr_units(*out["cexp_tab"], rr["rounded"]).max(),
              cexp_exact=cerr_units(*out["cexp_exact"], rr["exact_lo"]).max(),
              cexp_tab_exact=cerr_units(*out["cexp_tab_exact"], rr["exact"]).max(),
              big_tab_exact=cerr_units(*out["big_tab_exact"], br["tab"]).max(),
              big_poly_exact=cerr_units(*out["big_poly_exact"], br["poly"]).max())
    return mx, out


def measure_edges(on):
    """-> ({name: maximum error over every edge but x = -inf}, {name: True when x = -inf gave 0 or NaN / inf}, outputs)."""
    er = edge_refs()
    mx, minf, out = {}, {}, {}
    for name, xs, key in (("exp_neg", exp_edges(True), "exp_pos"), ("exp_neg_tab", exp_edges(), "exp")):
        out[name] = run_math(name, xs, on=on)
        keep = ~np.isneginf(xs)
        mx[name] = err_units(out[name][0], er[key])[keep].max()
        minf[name] = exp_minus_inf_ok(out[name][0], xs)
    xs = phase_edges("sincos")
    out["sincos_cw"] = run_math("sincos_cw", xs, on=on)
    mx["sincos_cw"] = max(err_units(out["sincos_cw"][0], er["sin"]).max(), err_units(out["sincos_cw"][1], er["cos"]).max())
    for form, names in (("poly", ("cexp", "cexp_exact")), ("tab", ("cexp_tab", "cexp_tab_exact"))):
        a, b, dt = cexp_edges(form)
        keep = ~np.isneginf(a)
        for name in names:
            out[name] = run_math(name, a, b, dt, on=on)
            mx[name] = cerr_units(*out[name], er[form])[keep].max()
            minf[name] = exp_minus_inf_ok(out[name][0], a) and exp_minus_inf_ok(out[name][1], a)
    return mx, minf, out


MIXED_LANES = (0, 37, 63)


def form_of(name):
    return "tab" if "tab" in name else "poly"


def run_mixed(name, lane, kind, on):
    a, b, dt, dt_lo = mixed_wave(form_of(name), lane, kind)
    return run_math(name, a, b, dt, dt_lo if name == "cexp_exact" else None, threads=64, on=on)


@functools.lru_cache(None)
def slow_lane_ref(name, lane):
    a, b, dt, dt_lo = (x[lane:lane + 1] for x in mixed_wave(form_of(name), lane, "slow"))
    if name.endswith("exact"):
        return ref_cexp(a, b, dt, dt_lo if name == "cexp_exact" else None, "exact")
    return ref_cexp(a, b, dt)


def measure_slow(on):
    """-> {name: maximum error of the one slow lane (0, 37, 63 in turn) of a wave of 64}."""
    mx = {}
    for name in COMPLEX_FORMS:
        mx[name] = 0.0
        for lane in MIXED_LANES:
            re, im = run_mixed(name, lane, "slow", on)
            mx[name] = max(mx[name], cerr_units(re[lane:lane + 1], im[lane:lane + 1], slow_lane_ref(name, lane)).max())
    return mx


# ---- (d) lane groups ----------------------------------------------------------------------------------------------------
GRP_IN, GRP_OUT = 4, 182
GO = dict(sum=0, max=1, partner=2, bc_c=3, bc_ci=19, bc_u=35, bc_iu=51, bcast=67, bcast_i=68, peek=69, peekk2=133, peek2=149,
          wave_all=181)


def grp_inputs(n, seed, special=False):
    """A different value in every lane: random mantissas, a sign, exponents spread over 2^+-40.  special: -0.0, a denormal,
    inf and a NaN with a payload sprinkled over every column (moves only: their sums are not compared)."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(1.0, 2.0, (n, GRP_IN)) * np.where(rng.random((n, GRP_IN)) < 0.5, -1.0, 1.0)
    v = np.ldexp(v, rng.integers(-40, 41, (n, GRP_IN)))
    iv = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    if special:
        sp = np.array([0x8000000000000000, 0x0000000000000123, 0x800fffffffffffff, 0x7ff0000000000000, 0xfff0000000000000,
                       0x7ff8000000abcdef, 0xfff4000000012345], dtype=np.uint64).view(np.float64)
        bits = v.view(np.uint64)
        for c in range(GRP_IN):
            where = rng.permutation(n)[:n // 3]
            bits[where, c] = sp[rng.integers(0, sp.size, where.size)].view(np.uint64)
        iv[rng.permutation(n)[:8]] = np.array([0, -1, 2 ** 31 - 1, -2 ** 31, 1, -2, 0x55555555, -0x55555556], dtype=np.int64).astype(np.int32)
    return v, iv


def _partners(n):
    i = np.arange(n)
    return [i ^ 1, i ^ 2, (i & ~7) | (7 - (i & 7)), (i & ~15) | (15 - (i & 15))]


def butterfly(v, G, op):
    """Grp<G>::sum / max: the partner order of grp_emu.h (xor 1, xor 2, half-mirror of 8, mirror of 16)."""
    v = np.array(v, dtype=np.float64)
    for stage, p in enumerate(_partners(v.size)):
        if G >= 2 << stage:
            v = op(v, v[p])
    return v


def grp_expected(G, v, iv, jsrc, flag):
    """Every output word of k_grp<G> (uint64), restated with numpy indexing."""
    n = v.shape[0]
    i = np.arange(n)
    gb = i & ~(G - 1)
    vb = v.view(np.uint64)
    ib = iv.view(np.uint32).astype(np.uint64)
    out = np.zeros((n, GRP_OUT), dtype=np.uint64)
    with np.errstate(all="ignore"):
        out[:, GO["sum"]] = butterfly(v[:, 0], G, np.add).view(np.uint64)
        out[:, GO["max"]] = butterfly(v[:, 0], G, np.fmax).view(np.uint64)
    out[:, GO["partner"]] = vb[i ^ 1, 0]
    for j in range(G):
        out[:, GO["bc_c"] + j] = out[:, GO["bc_u"] + j] = vb[gb + j, 0]
        out[:, GO["bc_ci"] + j] = out[:, GO["bc_iu"] + j] = ib[gb + j]
        out[:, GO["peek"] + 4 * j:GO["peek"] + 4 * j + 4] = vb[gb + j, :]
        out[:, GO["peekk2"] + j] = vb[gb + j, 1]
        out[:, GO["peek2"] + 2 * j] = vb[gb + j, 2]
        out[:, GO["peek2"] + 2 * j + 1] = vb[gb + j, 3]
    out[:, GO["bcast"]] = vb[gb + jsrc, 0]
    out[:, GO["bcast_i"]] = ib[gb + jsrc]
    out[:, GO["wave_all"]] = np.repeat(flag.reshape(-1, 64).all(axis=1), 64).astype(np.uint64)
    return out


def run_grp(G, v, iv, jsrc, flag, threads):
    n = v.shape[0]
    v, iv = _f64(v), np.ascontiguousarray(iv, dtype=np.int32)
    jsrc, flag = np.ascontiguousarray(jsrc, dtype=np.int32), np.ascontiguousarray(flag, dtype=np.int32)
    out = np.full((n, GRP_OUT), 0xdeadbeef, dtype=np.uint64)
    launch(device().devprim_grp, G, n, threads, _ptr(v), _ptr(iv, _ip), _ptr(jsrc, _ip), _ptr(flag, _ip), _ptr(out, _qp))
    return out


# ---- (e) row blocks ------------------------------------------------------------------------------------------------------
ROW_IN, ROW_OUT = 24, 18
RI = dict(c=0, s=1, D=2, ht=9, ct=10, scale=11, s0=12, S=13, k=20, nt=21, mu=22, z=23)
RO = dict(mm=0, w=7, var=8, k=9, S=10, innov=17)


def fma(a, b, c):
    """Correctly rounded a b + c (Python 3.10 has no math.fma): exact rational arithmetic, one rounding."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def row_inputs(n, seed):
    """Every per-lane input of k_row, different in every lane; magnitudes within 2^+-3 so that sums cancel partly."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(1.0, 2.0, (n, ROW_IN)) * np.where(rng.random((n, ROW_IN)) < 0.5, -1.0, 1.0)
    return np.ldexp(x, rng.integers(-3, 4, (n, ROW_IN)))


def run_row(P, x, e, y, threads=64):
    x = _f64(x)
    out = np.full((x.shape[0], ROW_OUT), np.nan)
    launch(device().devprim_row, P, x.shape[0], threads, _ptr(x), float(e), float(y), _ptr(out))
    return out


def row_colmix_ref(P, c, s, D):
    """grp_emu.h::row_colmix for one 16-lane row: mm_j = fma(-s@j, D_{j^1}, fma(c@j, D_j, 0)); the last column of an odd P
    has no second term.  c, s: [16]; D: [16, >= P] -> [16, P]."""
    mm = np.empty((16, P))
    for r in range(16):
        for j in range(P):
            m = fma(c[j], D[r, j], 0.0)
            if j < (P & ~1):
                m = fma(-s[j], D[r, j ^ 1], m)
            mm[r, j] = m
    return mm


def row_gain_ref(P, S, k, nt):
    """S_j += k@j nt: one fma."""
    return np.array([[fma(k[j], nt[r], S[r, j]) for j in range(P)] for r in range(16)])


def row_front_ref(P, x, e):
    """lazy_front of one row (lanes < P) in mpmath: w = sum_j S_j ht@j; t = ht w; k = w + ct; var = |e| scale + s0 + sum_j t@j.
    Returns {name: (value [P] as mpf, sum of the magnitudes of the terms [P] as float)}; var's terms are expanded down to the
    products S_i@j ht@i ht@j, since t@j carries the roundings of w@j."""
    f = lambda r, key, j=0: MP.mpf(float(x[r, RI[key] + j]))   # noqa: E731
    w, wmag = [], []
    for r in range(P):
        terms = [f(r, "S", j) * f(j, "ht") for j in range(P)]
        w.append(sum(terms))
        wmag.append(sum(abs(t) for t in terms))
    ae = abs(MP.mpf(float(e)))
    var, vmag, k, kmag = [], [], [], []
    for r in range(P):
        k.append(w[r] + f(r, "ct"))
        kmag.append(wmag[r] + abs(f(r, "ct")))
        var.append(ae * f(r, "scale") + f(r, "s0") + sum(f(j, "ht") * w[j] for j in range(P)))
        vmag.append(abs(ae * f(r, "scale")) + abs(f(r, "s0")) + sum(abs(f(j, "ht")) * wmag[j] for j in range(P)))
    return dict(w=(w, [float(m) for m in wmag]), k=(k, [float(m) for m in kmag]), var=(var, [float(m) for m in vmag]))


def row_innov_ref(P, x, y):
    """innov_t2 of one row: t = ht z; innov = y - mu - sum_j t@j."""
    f = lambda r, key: MP.mpf(float(x[r, RI[key]]))            # noqa: E731
    t = [f(j, "ht") * f(j, "z") for j in range(P)]
    val = [MP.mpf(float(y)) - f(r, "mu") - sum(t) for r in range(P)]
    mag = [float(abs(MP.mpf(float(y))) + abs(f(r, "mu")) + sum(abs(v) for v in t)) for r in range(P)]
    return val, mag


# ---- (f) RNG ---------------------------------------------------------------------------------------------------------------
PHILOX_KAT = (
    ((0, 0, 0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 6, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def run_philox(words, threads=256):
    words = np.ascontiguousarray(words, dtype=np.uint32)
    n = words.shape[0]
    out, u = np.zeros((n, 4), dtype=np.uint32), np.zeros(n)
    launch(device().devprim_philox, n, threads, _ptr(words, _up), _ptr(out, _up), _ptr(u))
    return out, u


@functools.lru_cache(None)
def rng_keys(n=4096, seed=99):
    """(key [n, 5] = k0 k1 chain purpose idx, iter [n]): random, with the edges of every field in the first rows."""
    rng = np.random.default_rng(seed)
    key = np.empty((n, 5), dtype=np.uint32)
    key[:, 0:3] = rng.integers(0, 2 ** 32, (n, 3), dtype=np.uint64)
    key[:, 3] = rng.integers(0, 4, n)
    key[:, 4] = rng.integers(0, 2 ** 23, n)
    it = rng.integers(0, 2 ** 48, n, dtype=np.uint64)
    iters = (0, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5)
    chains = (0, 2 ** 32 - 1)
    idxs = (0, 6, 13, 2 ** 23 - 1)
    r = 0
    for i_ in iters:
        for c_ in chains:
            for x_ in idxs:
                for p_ in range(4):
                    key[r] = (0x80000001 | (r * 2654435761 & 0x7fffffff), 0xf0000000 | r, c_, p_, x_)
                    it[r] = i_
                    r += 1
    key.setflags(write=False)
    it.setflags(write=False)
    return key, it


def run_rng(key, it, threads=256):
    key, it = np.ascontiguousarray(key, dtype=np.uint32), np.ascontiguousarray(it, dtype=np.uint64)
    out = np.zeros((key.shape[0], 3))
    launch(device().devprim_rng, key.shape[0], threads, _ptr(key, _up), _ptr(it, _qp), _ptr(out))
    return out


def u01_ref(hi, lo):
    """carma_rng.h u01: exact in double ((k + 0.5) 2^-53 with k < 2^53)."""
    return ((((int(hi) << 32) | int(lo)) >> 11) + 0.5) / 9007199254740992.0


@functools.lru_cache(None)
def rng_refs():
    """Per key: the uniform (exact double); the normal and the t8 variate in mpmath on the same Philox words, each with the
    bound of its test."""
    from carma_pack_amd import parallel as par
    key, it = rng_keys()
    n = key.shape[0]
    uni, z, zb, t8, tb = np.empty(n), Ref(n), np.empty(n), Ref(n), np.empty(n)
    two_pi = 2 * MP.pi
    s32 = MP.mpf(2) ** -32
    for i in range(n):
        k0, k1, chain, purpose, idx = (int(w) for w in key[i])
        c0, c1 = int(it[i]) & 0xffffffff, int(it[i]) >> 32
        x = par.philox4x32_10(c0, c1, chain, (purpose << 24) | idx, k0, k1)
        uni[i] = u01_ref(x[0], x[1])

        def normal(words):
            u1, u2 = MP.mpf(u01_ref(words[0], words[1])), MP.mpf(u01_ref(words[2], words[3]))
            rad = MP.sqrt(-2 * MP.log(u1))
            return rad * MP.cos(two_pi * u2), rad
        zv, rad = normal(par.philox4x32_10(c0, c1, chain, (3 << 24) | idx, k0, k1))
        z.put(i, zv, 1)
        zb[i] = 16 * U53 * float(rad)
        a = par.philox4x32_10(c0, c1, chain, 2 * idx, k0, k1)
        b = par.philox4x32_10(c0, c1, chain, 2 * idx + 1, k0, k1)
        zv, rad = normal(a)
        w = MP.mpf(1)
        for k in range(4):
            w *= (MP.mpf(b[k]) + MP.mpf(0.5)) * s32
        den = MP.sqrt(-2 * MP.log(w) / 8)
        tv = zv / den
        t8.put(i, tv, 1)
        tb[i] = float(16 * U53 * rad / den + 8 * U53 * abs(tv))
    return dict(uniform=uni, normal=z.freeze(), normal_bound=zb, t8=t8.freeze(), t8_bound=tb)


# ---- (g) reciprocals ------------------------------------------------------------------------------------------------------
RCP_RAW_BOUND = 2.0 ** -24                   # the project's figure is 2^-24.4 "(measured)" on another sample: 0.4 bit of room
# recip() and rsqrt_pos(): "~1 ulp" / "e^3 ~ 1e-22 plus one rounding".  The host build of carma_core.h divides (0.5 units), so there
# is no host maximum to add one unit to; the bar is a stated 2 units of 2^-53 |value|.
RECIP_UNITS = 2.0


@functools.lru_cache(None)
def binade_sweep(kind, n=20000, seed=424242):
    """Arguments over every binade whose result is a normal number (1 / x: 2^-1021 .. 2^1021, both signs; x^-1/2: every normal
    positive x), mantissas: 1, the last one of the binade, the neighbours of 2 (where x^-1/2 changes its table half), and a random
    sweep -- n values in all."""
    rng = np.random.default_rng(seed + len(kind))
    lo, hi = (-1021, 1021) if kind == "rcp" else (-1022, 1024)
    ex = np.arange(lo, hi)
    per = n // ex.size
    rest = n - per * ex.size
    e = np.r_[np.repeat(ex, per), rng.integers(lo, hi, rest)]
    mant = rng.uniform(1.0, 2.0, e.size)
    first = np.arange(0, per * ex.size, per)
    mant[first] = 1.0
    mant[first + 1] = np.nextafter(2.0, 0.0)
    mant[first + 2] = np.nextafter(1.0, 2.0)
    x = np.ldexp(mant, e)
    if kind == "rcp":
        x *= np.where(rng.random(x.size) < 0.5, -1.0, 1.0)
    assert x.size == n and np.isfinite(x).all()
    x.setflags(write=False)
    return x


@functools.lru_cache(None)
def recip_refs(kind):
    x = binade_sweep(kind)
    ref = Ref(x.size)
    for i, xi in enumerate(x):
        v = 1 / MP.mpf(float(xi)) if kind == "rcp" else 1 / MP.sqrt(MP.mpf(float(xi)))
        ref.put(i, v, abs(v) * U53)
    return ref.freeze()


# ---- (h) the merge of a two-sided evaluation (carma_pipew.h pipew_merge) ---------------------------------------------------
# An evaluation is (Da, a, Db, beta): forward half  z | y_a ~ N(a, V + Da), backward half  u | y_b ~ N(beta, V^-1 + Db);
# X = -Da, Y = -Db positive semidefinite, the eigenvalues of X Y in [0, 1).
MPM = mp.mp.clone()
MPM.dps = 120
MERGE_ORDERS = (2, 3, 4, 5, 6, 7)


def _proto():
    import sys
    d = os.path.join(HERE, "tools", "proto")
    if d not in sys.path:
        sys.path.insert(0, d)
    import two_sided
    return two_sided


def lower_sym(Da):
    """Da as the device reads it: the stored elements with row >= column, mirrored."""
    L = np.tril(np.asarray(Da, dtype=np.float64))
    return L + np.tril(L, -1).T


def merge_pack(P, slots, data_fill=0.0):
    """One wave of k_merge<P>: slots = two evaluations (or None: all zero) -> [64, P + 1].  Slot s: forward row 2 s, backward
    row 2 s + 1; lane ND + j of the forward row carries column j of Da and -a_j, of the backward row column j of Db and -beta_j."""
    ND = 16 - P
    x = np.zeros((64, P + 1))
    x[(np.arange(64) % 16) < ND] = data_fill
    for s, ev in enumerate(slots):
        if ev is None:
            continue
        Da, a, Db, beta = ev
        for j in range(P):
            x[32 * s + ND + j, :P] = Da[:, j]
            x[32 * s + ND + j, P] = -a[j]
            x[32 * s + 16 + ND + j, :P] = Db[:, j]
            x[32 * s + 16 + ND + j, P] = -beta[j]
    return x


def run_merge(P, x):
    """x [nblocks * 64, P + 1] -> [nblocks, 64, 2]: {acc.total(), the row pair's sum} per lane."""
    x = _f64(x)
    nb = x.shape[0] // 64
    assert nb >= 1 and x.shape == (nb * 64, P + 1)
    out = np.full((nb * 64, 2), -7.0)
    launch(device().devprim_merge, P, nb, _ptr(x), _ptr(out))
    return out.reshape(nb, 64, 2)


def merge_result(P, out, blk, slot):
    """-> (the evaluation's value: the pair sum in lane 0 of its forward row, the 32 lanes' words as uint64 [32, 2])."""
    w = out[blk, 32 * slot:32 * slot + 32]
    return float(w[0, 1]), np.ascontiguousarray(w).view(np.uint64)


class MergeTruth(object):
    """value (mpf, NaN where lambda_max >= 1), lam = lambda_max(X Y), kappa = 1 / (1 - lam), S = the sum of the magnitudes of
    the terms, U = 2^-53 kappa S."""
    __slots__ = ("value", "lam", "kappa", "S", "U")


def _lam_max_mp(X, Y, XY):
    """lambda_max(X Y): of the symmetric C^T X C where Y = C C^T is positive definite, else of X Y itself."""
    M = MPM
    P = X.rows
    if not any(XY[i, j] != 0 for i in range(P) for j in range(P)):
        return M.mpf(0)
    try:
        C_ = M.cholesky(Y)
        return max(M.eigsy(C_.T * X * C_, eigvals_only=True))
    except (ValueError, ZeroDivisionError):
        return max(M.re(v) for v in M.eig(XY, left=False, right=False))


def merge_truth(Da, a, Db, beta, units=True):
    """The closed form of two_sided.merge (N = I - Da Db) at 120 digits, from the doubles as the device reads them.  units=False:
    the value alone (NaN where det N <= 0)."""
    M = MPM
    P = len(a)
    X = -M.matrix(lower_sym(Da).tolist())
    Y = -M.matrix(np.asarray(Db, dtype=np.float64).tolist())
    av, bv = M.matrix([float(v) for v in a]), M.matrix([float(v) for v in beta])
    XY = X * Y
    N = M.eye(P) - XY
    out = MergeTruth()
    out.lam = _lam_max_mp(X, Y, XY) if units else M.nan
    LU, piv = M.LU_decomp(N)
    det = M.mpf(1)
    for i in range(P):
        det *= LU[i, i] * (-1 if i < len(piv) and piv[i] != i else 1)
    if (units and not out.lam < 1) or not det > 0:
        out.value, out.kappa, out.S, out.U = M.nan, M.inf, M.inf, M.inf
        return out
    solve = lambda b_: M.U_solve(LU, M.L_solve(LU, b_, piv))   # noqa: E731
    logdet = M.log(det)
    x1 = solve(av)
    x2 = solve(-(X * bv))                                     # N^-1 Da beta
    dot = lambda p_, q_: sum(p_[i] * q_[i] for i in range(P))  # noqa: E731
    out.value = -logdet / 2 + dot(bv, x1) + dot(bv, x2) / 2 - dot(Y * av, x1) / 2
    if not units:
        out.kappa = out.S = out.U = M.nan
        return out
    u = Y * av - bv
    s2 = dot(u, solve(X * u))                                 # |C^-1 L^T u|^2 = u . N^-1 X u
    out.kappa = 1 / (1 - out.lam)
    out.S = abs(logdet) / 2 + sum(abs(bv[j] * av[j]) for j in range(P)) + \
        sum(abs(av[i] * Y[i, j] * av[j]) for i in range(P) for j in range(P)) / 2 + abs(s2) / 2
    out.U = M.mpf(U53) * out.kappa * out.S
    return out


def merge_err(got, truth):
    """|got - truth| as an mpf; a truth of NaN wants NaN (0, else inf); a non-finite result of a finite truth is inf."""
    if MPM.isnan(truth.value):
        return MPM.mpf(0) if got != got else MPM.inf
    if not np.isfinite(got):
        return MPM.inf
    return abs(MPM.mpf(float(got)) - truth.value)


def merge_host(ev):
    """The float64 restatement (two_sided.merge_chol: the device's algorithm) on what the device reads."""
    Da, a, Db, beta = ev
    with np.errstate(all="ignore"):
        return float(_proto().merge_chol(lower_sym(Da), np.asarray(a, float), np.asarray(Db, float), np.asarray(beta, float)))


def _sym_psd(rng, P, r=None):
    B = rng.standard_normal((P, P if r is None else r))
    M_ = B @ B.T
    return np.tril(M_) + np.tril(M_, -1).T                    # symmetric bit for bit


def _lam_max(X, Y):
    w = np.linalg.eigvals(X @ Y).real
    return float(w.max())


def _scaled_y(rng, X, lam):
    """A random positive semidefinite Y with lambda_max(X Y) = lam (to rounding); X = 0: any Y."""
    P = X.shape[0]
    Y = _sym_psd(rng, P)
    top = _lam_max(X, Y)
    return Y * (lam / top) if top > 0 else Y


MERGE_LAMS = (0.3, 0.99, 1.0 - 1e-6)
MERGE_DRAWS = 8


def _embed(P, X2):
    X = np.zeros((P, P))
    X[:2, :2] = X2
    return X


@functools.lru_cache(None)
def merge_cases(P):
    """The synthetic families: [(family, evaluation)].  family "rank0" has the derived bar, "delta-small" the widened one (its
    partner "delta-zero" is the same evaluation at delta = 0), every other one the measured factor HOST_MAX["merge"][P]."""
    rng = np.random.default_rng(6100 + P)
    cases = []
    for r in range(P + 1):
        for lam in MERGE_LAMS:
            for _ in range(MERGE_DRAWS):
                X = _sym_psd(rng, P, r)
                Y = _scaled_y(rng, X, lam)
                cases.append(("rank0" if r == 0 else "rank%d" % r, (-X, rng.standard_normal(P), -Y, rng.standard_normal(P))))
    for lam in MERGE_LAMS:
        for _ in range(2):
            # every pivot a tie: a unit diagonal (a correlation matrix, scaled by exact powers of two) and 3 I
            X = _sym_psd(rng, P)
            d = 2.0 ** -np.round(0.5 * np.log2(np.diag(X)))
            X = X * d[:, None] * d[None, :]
            X = X / np.sqrt(np.outer(np.diag(X), np.diag(X)))
            X = np.tril(X) + np.tril(X, -1).T
            np.fill_diagonal(X, 1.0)
            if np.linalg.eigvalsh(X).min() > 1e-3:
                cases.append(("unit-diagonal", (-X, rng.standard_normal(P), -_scaled_y(rng, X, lam), rng.standard_normal(P))))
            X = 3.0 * np.eye(P)
            cases.append(("3I", (-X, rng.standard_normal(P), -_scaled_y(rng, X, lam), rng.standard_normal(P))))
        # a pivot just above the rank cut (taken), just below it (either decision passes), and the same at delta = 0
        a, beta = rng.standard_normal(P), rng.standard_normal(P)
        Y = _scaled_y(rng, _embed(P, [[1.0, 1.0], [1.0, 1.0]]), lam)
        for name, delta in (("delta-large", 4e-14), ("delta-small", 4e-16), ("delta-zero", 0.0)):
            cases.append((name, (-_embed(P, [[1.0, 1.0], [1.0, 1.0 + delta]]), a, -Y, beta)))
        # a diagonal entry at -1e-17 with a zero row and column
        X = _sym_psd(rng, P, P - 1)
        X[P - 1, :] = X[:, P - 1] = 0.0
        X[P - 1, P - 1] = -1e-17
        cases.append(("negative-diagonal", (-X, rng.standard_normal(P), -_scaled_y(rng, X, lam), rng.standard_normal(P))))
    for _, ev in cases:
        for arr in ev:
            arr.setflags(write=False)
    return tuple(cases)


@functools.lru_cache(None)
def merge_truths(P):
    return tuple(merge_truth(*ev) for _, ev in merge_cases(P))


def merge_allowance(P, factor):
    """Per case of merge_cases(P): the allowed |result - truth| (float).  rank0: (P + 2) 2^-53 S -- the result is
    beta.a - 1/2 a.Y a, P + 2 roundings of partial sums that S bounds.  delta-small: factor U + |truth(delta) - truth(0)|.
    Otherwise factor U."""
    cases, truths = merge_cases(P), merge_truths(P)
    out = []
    for i, (fam, _) in enumerate(cases):
        t = truths[i]
        if fam == "rank0":
            out.append(float((P + 2) * U53 * t.S))
        elif fam == "delta-small":
            assert cases[i + 1][0] == "delta-zero"
            out.append(float(factor * t.U + abs(t.value - truths[i + 1].value)))
        else:
            out.append(float(factor * t.U))
    return np.array(out)


def merge_measure(P, results):
    """results: one value per case -> (largest |result - truth| / U over the families with the measured factor,
    largest |result - truth| / ((P + 2) 2^-53 S) over rank 0, errors [n] as floats)."""
    cases, truths = merge_cases(P), merge_truths(P)
    err = np.array([float(merge_err(results[i], truths[i])) for i in range(len(cases))])
    worst, worst0 = 0.0, 0.0
    for i, (fam, _) in enumerate(cases):
        if fam == "rank0":
            worst0 = max(worst0, err[i] / float((P + 2) * U53 * truths[i].S))
        elif fam != "delta-small":
            worst = max(worst, err[i] / float(truths[i].U))
    return worst, worst0, err


# ---- inputs of the merge from real half filters
REAL_ORDERS = ((2, 1), (5, 3), (7, 6))
REAL_N = (6, 20, 41, 120)
REAL_DRAWS = 8
COINCIDENT = (3, 1, 120, 34, (17.05379556956296, 1.2281142449115867, 35.43706442791335, -5.014528819389739, -1.7473257300527083,
                              -2.87620882248127, 18.963673587819525))     # test_state_with_nearly_coincident_real_roots


def _halves(t, y, yerr, theta, p, q):
    """(l_a, Da, a, l_b, Db, beta) of two_sided.loglik_two_sided at the device's split and meeting time."""
    ts = _proto()
    om, h, Vz, pairs = ts.real_model(theta, p, q)
    n = t.size
    m = (n + 1) // 2
    yc, e = y - theta[2], theta[1] * yerr ** 2
    c, s0 = Vz @ h, h @ Vz @ h
    la, Da, a = ts.half_filter(om, pairs, p, h, c, s0, t[:m], yc[:m], e[:m], t[m - 1], False)
    lb, Db, beta = ts.half_filter(om, pairs, p, c, h, s0, t[m:][::-1], yc[m:][::-1], e[m:][::-1], t[m - 1], True)
    return la, Da, a, lb, Db, beta


@functools.lru_cache(None)
def real_cases(p):
    """[(l_a + l_b, evaluation)] of order p: prior-like draws on irregular series of every length of REAL_N (and, at p = 3, the
    state with two real roots 6e-4 apart)."""
    from carma_pack_amd.synth import irregular_series, prior_like_theta
    out = []
    todo = []
    for (pp, q) in REAL_ORDERS:
        if pp == p:
            rng = np.random.default_rng(9000 + p)
            for n in REAL_N:
                t, y, yerr = irregular_series(n, seed=50 + n)
                k = 0
                while k < REAL_DRAWS:
                    todo.append((t, y, yerr, prior_like_theta(rng, p, q, t, y), q))
                    k += 1
    if p == COINCIDENT[0]:
        t, y, yerr = irregular_series(COINCIDENT[2], seed=COINCIDENT[3])
        todo.append((t, y, yerr, np.array(COINCIDENT[4]), COINCIDENT[1]))
    for t, y, yerr, th, q in todo:
        with np.errstate(all="ignore"):
            la, Da, a, lb, Db, beta = _halves(t, y, yerr, th, p, q)
        if not (np.isfinite(la + lb) and np.isfinite(Da).all() and np.isfinite(Db).all()):
            continue
        ev = (Da, a, Db, beta)
        for arr in ev:
            arr.setflags(write=False)
        out.append((float(la + lb), ev))
    return tuple(out)


REAL_P = (2, 3, 5, 7)


@functools.lru_cache(None)
def real_truths(p):
    return tuple(merge_truth(*ev, units=False) for _, ev in real_cases(p))


def real_measure(p, results):
    """Largest |result - truth| / |l_a + l_b + truth| over real_cases(p) (evaluations whose truth is NaN want NaN)."""
    worst = 0.0
    for i, (lab, _) in enumerate(real_cases(p)):
        t = real_truths(p)[i]
        e = merge_err(results[i], t)
        worst = max(worst, float(e if MPM.isnan(t.value) else e / abs(lab + t.value)))
    return worst


REAL_FLOOR = 16 * U53                    # the P + 2 additions into a sum of the size of the whole log-likelihood


# ---- (i) the window blocks (carma_win_asm.h, generated by tools/gen_win_asm.py) -------------------------------------------
WIN_EPS_T = 2.0 ** -48                   # t = -G / m@j: v_rcp_f64 to 2^-24.4, one Newton step leaves (2^-24.4)^2, + two roundings
RCP_REL = 2.0 ** -24.4


def win_init_inputs(P, seed, nblocks=1):
    """[nblocks * 64, 3 P + 2]: kn[P], nun, kk[P], nuF, hn[P], every lane its own values."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(1.0, 2.0, (nblocks * 64, 3 * P + 2)) * np.where(rng.random((nblocks * 64, 3 * P + 2)) < 0.5, -1.0, 1.0)
    return np.ldexp(x, rng.integers(-3, 4, x.shape))


def run_win_init(P, x):
    x = _f64(x)
    nb = x.shape[0] // 64
    assert nb >= 1 and x.shape == (nb * 64, 3 * P + 2)
    out = np.full((nb * 64, P + 1), np.nan)
    launch(device().devprim_win_init, P, nb, _ptr(x), _ptr(out))
    return out


def win_init_ref(P, x):
    """WinAsm<P>::init on one row x [16, 3 P + 2] -> [16, P + 1]: the FMA chain in the generator's order (s outer, r inner);
    kk_r and nuF come from the virtual lane ND + s."""
    ND = 16 - P
    out = np.empty((16, P + 1))
    for l in range(16):
        kn, nun = [x[l, r] for r in range(P)], x[l, P]
        for s in range(P):
            hs = x[l, 2 * P + 2 + s]
            for r in range(P):
                kn[r] = fma(x[ND + s, P + 1 + r], hs, kn[r])
            nun = fma(x[ND + s, 2 * P + 1], hs, nun)
        out[l, :P], out[l, P] = kn, nun
    return out


def win_chunk_inputs(P, seed, noise=1.0, gain=0.0, nblocks=1):
    """[nblocks * 64, 2 P + 2]: kk[P], hh[P], m, nu of a chunk as start() leaves it, four independent rows per wave: data lane j
    h_j random, kk_j = S h_j + c_j, m_j = e_j + h_j . kk_j, nu_j random; virtual lane s: hh = e_s, kk = column s of S (positive
    semidefinite), m = 1 + S_ss, nu = -z_s.  noise: the size of e_j (small: the pivots cancel); gain: the size of V in c_j = V h_j
    (V positive semidefinite, so that the chunk's covariance H (S + V) H^T + diag(e) is positive definite: every pivot > 0)."""
    ND = 16 - P
    rng = np.random.default_rng(seed)
    x = np.zeros((nblocks * 64, 2 * P + 2))
    for row in range(nblocks * 4):
        A = rng.standard_normal((P, P))
        S = A @ A.T / P
        S = np.tril(S) + np.tril(S, -1).T
        B = rng.standard_normal((P, P))
        V = gain * (B @ B.T) / P
        V = np.tril(V) + np.tril(V, -1).T
        o = x[16 * row:16 * row + 16]
        for j in range(ND):
            h = rng.standard_normal(P)
            kk = S @ h + V @ h
            o[j, :P], o[j, P:2 * P] = kk, h
            o[j, 2 * P] = noise * rng.uniform(0.5, 1.5) + h @ kk
            o[j, 2 * P + 1] = rng.standard_normal()
        for s in range(P):
            o[ND + s, :P] = S[:, s]
            o[ND + s, P + s] = 1.0
            o[ND + s, 2 * P] = 1.0 + S[s, s]
            o[ND + s, 2 * P + 1] = rng.standard_normal()
    return x


def win_neutral_inputs(P, seed):
    """A chunk of neutral slots: data lanes hh = kk = 0, m = 1, nu = 0; the virtual lanes as in win_chunk_inputs."""
    ND = 16 - P
    x = win_chunk_inputs(P, seed)
    data = (np.arange(64) % 16) < ND
    x[data] = 0.0
    x[data, 2 * P] = 1.0
    return x


WIN_FILL = -12345.0                      # what a lane that stores nothing leaves in the output array


def run_win_chunk(P, x, rows=None):
    """-> (out [n, P + 4]: kk[P], mA, mB, nuA, nuB; marker [n]).  rows: the call under `if (row active)`, bit q = row q of every wave."""
    x = _f64(x)
    nb = x.shape[0] // 64
    assert nb >= 1 and x.shape == (nb * 64, 2 * P + 2)
    out = np.full((nb * 64, P + 4), WIN_FILL)
    marker = np.zeros(nb * 64, dtype=np.int32)
    if rows is None:
        launch(device().devprim_win_chunk, P, nb, _ptr(x), _ptr(out), _ptr(marker, _ip))
    else:
        launch(device().devprim_win_chunk_masked, P, nb, int(rows), _ptr(x), _ptr(out), _ptr(marker, _ip))
    return out, marker


def win_chunk_truth(P, x):
    """The elimination of one row x [16, 2 P + 2] in mpmath, every lane and register as the block leaves it:
        for j = 0 .. ND-1, in the lanes l >= j:  G = sum_r kk_r@j hh_r ;  t = -G / m@j ;  m' = m + G t ;  nu' = nu + nu@j t ;
                                                 kk_r += kk_r@j t          (m, nu: pivot j reads A / B for j even / odd, writes the other)
    with a running bound of the device's error per register, to first order in the rounding unit u = 2^-53: G takes P roundings
    (each at most u times a partial sum, which the sum of the magnitudes bounds), the updates of m, nu and kk_r one each, t carries
    the relative error WIN_EPS_T; errors of the operands go through the derivatives' magnitudes.
    -> (val, err): [16, P + 4] object arrays of mpf, columns as run_win_chunk's."""
    ND = 16 - P
    f = lambda v: MP.mpf(float(v))                             # noqa: E731
    u, et_rel = MP.mpf(U53), MP.mpf(WIN_EPS_T)
    K = [[f(x[l, r]) for r in range(P)] for l in range(16)]
    eK = [[MP.mpf(0)] * P for _ in range(16)]
    H = [[f(x[l, P + r]) for r in range(P)] for l in range(16)]
    M_ = [[f(x[l, 2 * P]) for l in range(16)] for _ in range(2)]
    NU = [[f(x[l, 2 * P + 1]) for l in range(16)] for _ in range(2)]
    eM = [[MP.mpf(0)] * 16 for _ in range(2)]
    eNU = [[MP.mpf(0)] * 16 for _ in range(2)]
    for j in range(ND):
        cur, alt = j & 1, 1 - (j & 1)
        kj, ekj = list(K[j]), list(eK[j])
        mj, emj, nj, enj = M_[cur][j], eM[cur][j], NU[cur][j], eNU[cur][j]
        for l in range(j, 16):
            terms = [kj[r] * H[l][r] for r in range(P)]
            G = sum(terms)
            eG = sum(abs(H[l][r]) * ekj[r] for r in range(P))
            eG += P * u * (sum(abs(v) for v in terms) + eG)
            t = -G / mj
            et = eG / abs(mj) + abs(G) * emj / (mj * mj)
            et += et_rel * (abs(t) + et)
            mn = M_[cur][l] + G * t
            e = eM[cur][l] + abs(t) * eG + abs(G) * et + eG * et
            M_[alt][l], eM[alt][l] = mn, e + u * (abs(mn) + e)
            nn = NU[cur][l] + nj * t
            e = eNU[cur][l] + abs(t) * enj + abs(nj) * et + enj * et
            NU[alt][l], eNU[alt][l] = nn, e + u * (abs(nn) + e)
            for r in range(P):
                kn = K[l][r] + kj[r] * t
                e = eK[l][r] + abs(t) * ekj[r] + abs(kj[r]) * et + ekj[r] * et
                K[l][r], eK[l][r] = kn, e + u * (abs(kn) + e)
    val = np.empty((16, P + 4), dtype=object)
    err = np.empty((16, P + 4), dtype=object)
    for l in range(16):
        val[l, :P], err[l, :P] = K[l], eK[l]
        val[l, P:] = [M_[0][l], M_[1][l], NU[0][l], NU[1][l]]
        err[l, P:] = [eM[0][l], eM[1][l], eNU[0][l], eNU[1][l]]
    return val, err


def win_chunk_f64(P, x, newton=True):
    """The instruction sequence of WinAsm<P>::chunk on one row in float64 (correctly rounded FMAs), with v_rcp_f64 replaced by
    the division moved by the full 2^-24.4 the project states for it, the sign alternating.  newton=False: without the Newton
    step folded into t (a wrong block, for the test of the bound).  -> [16, P + 4]."""
    ND = 16 - P
    K = [[float(x[l, r]) for r in range(P)] for l in range(16)]
    H = [[float(x[l, P + r]) for r in range(P)] for l in range(16)]
    M_ = [[float(x[l, 2 * P]) for l in range(16)] for _ in range(2)]
    NU = [[float(x[l, 2 * P + 1]) for l in range(16)] for _ in range(2)]
    for j in range(ND):
        cur, alt = j & 1, 1 - (j & 1)
        kj, rb, bnu = list(K[j]), M_[cur][j], NU[cur][j]
        for l in range(j, 16):
            G = 0.0
            for r in range(P):
                G = fma(kj[r], H[l][r], G)
            r0 = (1.0 / rb) * (1.0 + (RCP_REL if (j + l) & 1 else -RCP_REL))
            e = fma(-rb, r0, 1.0)
            t = G * -r0
            if newton:
                t = fma(t, e, t)
            M_[alt][l] = fma(G, t, M_[cur][l])
            NU[alt][l] = fma(bnu, t, NU[cur][l])
            for r in range(P):
                K[l][r] = fma(kj[r], t, K[l][r])
    out = np.empty((16, P + 4))
    for l in range(16):
        out[l, :P] = K[l]
        out[l, P:] = [M_[0][l], M_[1][l], NU[0][l], NU[1][l]]
    return out


def win_checked(P):
    """(lane, column) of what the tests hold to the truth: each data lane's final variance and innovation (mA / nuA for an even
    lane, mB / nuB for an odd one), the virtual lanes' kk (the columns of S) and their nu in the register the last pivot wrote."""
    ND = 16 - P
    cells = []
    for j in range(ND):
        cells += [(j, P + (j & 1)), (j, P + 2 + (j & 1))]
    for s in range(P):
        cells += [(ND + s, r) for r in range(P)] + [(ND + s, P + 2 + (ND & 1))]
    return cells


def win_chunk_worst(P, got, val, err):
    """Largest |got - truth| / bound over win_checked(P) (a bound of 0 wants the exact value)."""
    worst = 0.0
    for l, c in win_checked(P):
        d = abs(MP.mpf(float(got[l, c])) - val[l, c])
        if not np.isfinite(got[l, c]):
            return np.inf
        worst = max(worst, float(d / err[l, c]) if err[l, c] > 0 else (0.0 if d == 0 else np.inf))
    return worst
