"""Builds and loads the device-primitive harness (tests/devprim/devprim.hip) and the host build of carma_math.h
(tests/devprim/hostmath.cpp); the argument arrays of the primitive tests; their references, mpmath at 50 digits and numpy
restatements of grp_device.h / carma_row_asm.h / carma_rng.h.  Test code only."""
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
DEV_HEADERS = ("grp_device.h", "carma_types.h", "carma_row_asm.h", "carma_math.h", "carma_math_tab.h", "carma_rng.h")

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
    # _share_hip_runtime_with_torch); loading this harness first would map the system's and leave the product without devices
    import carma_pack_amd._lib  # noqa: F401
    L = C.CDLL(build_device())
    L.devprim_math.argtypes = [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]
    L.devprim_grp.argtypes = [C.c_int, C.c_int, C.c_int, _dp, _ip, _ip, _ip, _qp]
    L.devprim_row.argtypes = [C.c_int, C.c_int, C.c_int, _dp, C.c_double, C.c_double, _dp]
    L.devprim_philox.argtypes = [C.c_int, C.c_int, _up, _up, _dp]
    L.devprim_rng.argtypes = [C.c_int, C.c_int, _up, _qp, _dp]
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


FN = dict(exp_neg=0, exp_neg_tab=1, sincos_cw=2, cexp=3, cexp_tab=4, cexp_exact=5, cexp_tab_exact=6)
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
