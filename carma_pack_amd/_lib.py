"""ctypes binding of libcarma_mi355.so (the C ABI declared in include/carma_mi355.h).

This is the ONLY route from Python to the compute path.  There is no CPU fallback: if the
shared library is missing the import fails, and without a gfx950 device every compute call
raises ``CarmaDeviceError``.

Layout: SIGNATURES (the C ABI, once), the small marshalling helpers every wrapper uses, the handle base and the sampler
mixin, then the classes and the stateless calls.  Every wrapper names the C function it calls and spells out its arguments.
"""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CARMA_LIB_PATH: another build of the same C ABI (A/B measurements of kernel variants); default: the in-tree build
LIB_PATH = os.environ.get("CARMA_LIB_PATH") or os.path.join(_HERE, "libcarma_mi355.so")

CARMA_OK, CARMA_EINVAL, CARMA_ENODEV, CARMA_ENOMEM, CARMA_EHIP = 0, -22, -19, -12, -5
PMAX = 7

_dp, _ip, _lp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_long)
_ullp = C.POINTER(C.c_ulonglong)
_I, _L, _D, _V, _S, _U64 = C.c_int, C.c_long, C.c_double, C.c_void_p, C.c_char_p, C.c_uint64
_SERIES = [_dp, _dp, _dp, _I]                                    # time, y, yerr, n
_MLE_TAIL = [_I, _I, _D, _D, _D, _I, _V, _V, _V, _V, _V]         # maxiter ... ignore_prior, x, fun, nit, nfev, status
_ITEMS = [_V, _ip, _I, _dp, _dp, _dp, _I, _dp]                   # handle, which, M, sigsqr, roots, ma, nma, mu
_AT_TIMES = _ITEMS + [_dp, _lp, _dp, _dp, _ip]                   # ... times, toff, mean, var, singular

# name -> (restype, argtypes): every function include/carma_mi355.h declares.  _load() applies it, EXPORTS is its keys, and
# tests/test_capi_signatures_cpu.py holds it to the header.  c_void_p entries take device addresses as integers (the _dev
# entry points) or are called by tests and tools with data_as(c_void_p): they stay c_void_p.
SIGNATURES = {
    "carma_version": (_S, []),
    "carma_last_error": (_S, []),
    "carma_device_count": (_I, []),
    "carma_tune_set": (_I, [_S, _L]),
    "carma_ctx_create": (_V, _SERIES + [_I, _I, _D, _I]),
    "carma_ctx_destroy": (None, [_V]),
    "carma_ctx_n": (_I, [_V]),
    "carma_ctx_dim": (_I, [_V]),
    "carma_ctx_get_data": (_I, [_V, _dp, _dp, _dp]),
    "carma_ctx_get_prior": (_I, [_V, _dp]),
    "carma_ctx_set_prior": (_I, [_V, _D]),
    "carma_logdensity_batch": (_I, [_V, _dp, _I, _I, _dp]),
    "carma_logdensity_batch_dev": (_I, [_V, _V, _I, _I, _V, _V]),
    "carma_logdensity_kernel_name": (_I, [_V, _I, _S, _I]),
    "carma_logprior": (_D, [_V, _dp]),
    "carma_mle_batched": (_I, [_V, _V, _I, _V, _V] + _MLE_TAIL),
    "carma_mctx_create": (_V, [_dp, _dp, _dp, _lp, _I, _I, _I, _dp, _I]),
    "carma_mctx_destroy": (None, [_V]),
    "carma_mctx_nseries": (_I, [_V]),
    "carma_mctx_dim": (_I, [_V]),
    "carma_mctx_n": (_I, [_V, _I]),
    "carma_mctx_get_data": (_I, [_V, _I, _dp, _dp, _dp]),
    "carma_mctx_get_prior": (_I, [_V, _I, _dp]),
    "carma_mlogdensity_batch": (_I, [_V, _dp, _ip, _I, _I, _dp]),
    "carma_mlogdensity_kernel_name": (_I, [_V, _S, _I]),
    "carma_mkfilter": (_I, _ITEMS + [_dp, _dp, _lp, _ip]),
    "carma_mpredict": (_I, _AT_TIMES),
    "carma_msmooth": (_I, _AT_TIMES),
    "carma_mle_batched_ms": (_I, [_V, _V, _V, _I, _V, _V] + _MLE_TAIL),
    "carma_bands_create": (_V, [_dp, _dp, _dp, _lp, _I, _I, _I, _dp, _dp, _D, _I]),
    "carma_bands_destroy": (None, [_V]),
    "carma_bands_dim": (_I, [_V]),
    "carma_bands_nbands": (_I, [_V]),
    "carma_bands_n": (_I, [_V, _I]),
    "carma_bands_get_prior": (_I, [_V, _dp]),
    "carma_bands_logdensity_batch": (_I, [_V, _dp, _I, _I, _dp]),
    "carma_bands_logdensity_batch_dev": (_I, [_V, _V, _I, _I, _V, _V]),
    "carma_bands_mle_batched": (_I, [_V, _V, _I, _V, _V, _V] + _MLE_TAIL),
    "carma_bands_smooth": (_I, [_V, _dp, _I, _I, _dp, _I, _dp, _dp, _dp, _dp, _ip]),
    "carma_bandset_create": (_V, [_dp, _dp, _dp, _lp, _I, _I, _I, _I, _dp, _dp, _dp, _I]),
    "carma_bandset_destroy": (None, [_V]),
    "carma_bandset_nobjects": (_I, [_V]),
    "carma_bandset_nbands": (_I, [_V]),
    "carma_bandset_dim": (_I, [_V]),
    "carma_bandset_n": (_I, [_V, _I, _I]),
    "carma_bandset_get_prior": (_I, [_V, _I, _dp]),
    "carma_bandset_logdensity_batch": (_I, [_V, _dp, _ip, _I, _I, _dp]),
    "carma_bandset_kernel_name": (_I, [_V, _S, _I]),
    "carma_bandset_mle_batched": (_I, [_V, _V, _V, _I, _V, _V, _V] + _MLE_TAIL),
    "carma_bandset_smooth": (_I, [_V, _dp, _ip, _ip, _I, _dp, _lp, _dp, _dp, _ip]),
    "carma_bands_pt_default_box": (_I, [_V, _dp, _dp]),
    "carma_bands_pt_create": (_I, [_V, _I, _I, _dp, _I, _U64, _dp, _dp]),
    "carma_bands_pt_start": (_I, [_V, _dp]),
    "carma_bands_pt_set_chains": (_I, [_V, _dp, _dp]),
    "carma_bands_pt_get_chains": (_I, [_V, _dp, _dp]),
    "carma_bands_pt_get_factor": (_I, [_V, _dp]),
    "carma_bands_pt_set_factor": (_I, [_V, _dp]),
    "carma_bands_pt_iterate": (_I, [_V, _L, _I]),
    "carma_bands_pt_sample": (_I, [_V, _I, _I, _dp, _dp]),
    "carma_bands_pt_stats": (_I, [_V, _dp, _dp, _I]),
    "carma_bands_pt_iterations_done": (_L, [_V]),
    "carma_bands_pt_logdensity": (_I, [_V, _dp, _dp]),
    "carma_bands_pt_kernel_name": (_I, [_V, _S, _I]),
    "carma_bands_pt_run": (_I, [_V, _I, _I, _I, _I, _I, _dp, _U64, _dp, _dp, _dp, _dp]),
    "carma_bandset_pt_default_box": (_I, [_V, _I, _dp, _dp]),
    "carma_bandset_pt_create": (_I, [_V, _ip, _I, _I, _I, _dp, _I, _U64, _dp, _dp]),
    "carma_bandset_pt_start": (_I, [_V, _dp]),
    "carma_bandset_pt_set_chains": (_I, [_V, _dp, _dp]),
    "carma_bandset_pt_get_chains": (_I, [_V, _dp, _dp]),
    "carma_bandset_pt_get_factor": (_I, [_V, _dp]),
    "carma_bandset_pt_set_factor": (_I, [_V, _dp]),
    "carma_bandset_pt_iterate": (_I, [_V, _L, _I]),
    "carma_bandset_pt_sample": (_I, [_V, _I, _I, _dp, _dp]),
    "carma_bandset_pt_stats": (_I, [_V, _dp, _dp, _I]),
    "carma_bandset_pt_iterations_done": (_L, [_V]),
    "carma_bandset_pt_logdensity": (_I, [_V, _dp, _dp]),
    "carma_bandset_pt_kernel_name": (_I, [_V, _S, _I]),
    "carma_bandset_pt_run": (_I, [_V, _ip, _I, _I, _I, _I, _I, _I, _dp, _U64, _dp, _dp, _dp, _dp]),
    "carma_kfilter_carma": (_I, _SERIES + [_I, _D, _dp, _dp, _I, _dp, _dp, _ip, _I]),
    "carma_kfilter_batch_carma": (_I, _SERIES + [_I, _I, _dp, _dp, _dp, _I, _dp, _dp, _dp, _ip, _ip, _I]),
    "carma_kfilter_car1": (_I, _SERIES + [_D, _D, _dp, _dp, _ip, _I]),
    "carma_predict_carma": (_I, _SERIES + [_I, _D, _dp, _dp, _I, _dp, _I, _dp, _dp, _I]),
    "carma_predict_car1": (_I, _SERIES + [_D, _D, _dp, _I, _dp, _dp, _I]),
    "carma_normalize_roots": (_I, [_I, _dp, _dp]),
    "carma_kf_create_carma": (_V, _SERIES + [_I, _D, _dp, _dp, _I, _I]),
    "carma_kf_create_car1": (_V, _SERIES + [_D, _D, _I]),
    "carma_kf_destroy": (None, [_V]),
    "carma_kf_n": (_I, [_V]),
    "carma_kf_filter": (_I, [_V, _dp, _dp]),
    "carma_kf_predict": (_I, [_V, _dp, _I, _dp, _dp]),
    "carma_simulate_carma": (_I, [_dp, _I, _I, _D, _dp, _dp, _I, _I, _U64, _dp, _I]),
    "carma_simulate_car1": (_I, [_dp, _I, _D, _D, _I, _U64, _dp, _I]),
    "carma_simulate_cond_carma": (_I, _SERIES + [_I, _I, _dp, _dp, _dp, _I, _dp, _dp, _I, _U64, C.c_uint, _dp, _dp, _dp, _ip,
                                                 _ip, _I]),
    "carma_simulate_cond_car1": (_I, _SERIES + [_I, _dp, _dp, _dp, _dp, _I, _U64, C.c_uint, _dp, _dp, _dp, _ip, _ip, _I]),
    "carma_smooth_carma": (_I, _SERIES + [_I, _I, _dp, _dp, _dp, _I, _dp, _dp, _I, _dp, _dp, _dp, _dp, _ip, _ip, _I]),
    "carma_smooth_car1": (_I, _SERIES + [_I, _dp, _dp, _dp, _dp, _I, _dp, _dp, _dp, _dp, _ip, _ip, _I]),
    "carma_sigma_noise_batch": (_I, [_I, _I, _dp, _dp, _dp, _I, _dp, _I]),
    "carma_psd_band": (_I, [_I, _I, _dp, _dp, _dp, _I, _dp, _I, _dp, _I, _dp, _dp, _I]),
    "carma_mpsd_band": (_I, [_I, _I, _dp, _dp, _dp, _lp, _I, _dp, _I, _dp, _I, _dp, _I]),
    "carma_mpsd_fused_max": (_I, []),
    "carma_mpsd_freq_tile": (_I, []),
    "carma_chain_diag": (_I, [_dp, _L, _I, _L, _I, _dp, _dp, _dp, _ip, _dp, _I]),
    "carma_chain_diag_dmax": (_I, []),
    "carma_chain_diag_kernel_ms": (_D, []),
    "carma_pt_run": (_I, [_V, _I, _I, _I, _I, _I, _dp, _I, _U64, _dp, _dp]),
    "carma_pt_create": (_I, [_V, _I, _I, _dp, _I, _U64]),
    "carma_pt_shard": (_I, [_V, _I, _I, _I]),
    "carma_pt_bind_state": (_I, [_V, _V, _V]),
    "carma_pt_start": (_I, [_V, _dp, _I]),
    "carma_pt_set_chains": (_I, [_V, _dp, _dp]),
    "carma_pt_get_chains": (_I, [_V, _dp, _dp]),
    "carma_pt_get_factor": (_I, [_V, _dp]),
    "carma_pt_set_factor": (_I, [_V, _dp]),
    "carma_pt_iterate": (_I, [_V, _L, _I]),
    "carma_pt_sample": (_I, [_V, _I, _I, _dp, _dp]),
    "carma_pt_stats": (_I, [_V, _dp, _dp, _I]),
    "carma_pt_iterations_done": (_L, [_V]),
    "carma_pt_iterate_sharded": (_I, [C.POINTER(_V), _I, _L, _V]),
    "carma_pt_sample_sharded": (_I, [C.POINTER(_V), _I, _I, _I, _V, _dp, _dp]),
    "carma_pt_boundary_stats": (_I, [_V, _ullp, _ullp]),
    "carma_pt_boundary_check": (_I, [_V]),
    "carma_pt_kernel_in_use": (_I, [_V]),
    "carma_pt_row_pipeline": (_I, []),
    "carma_pt_sweep": (_I, [_V]),
    "carma_pt_debug_draws": (_I, [_V, _I, _I, C.c_ulonglong, _dp, _dp, _dp]),
    "carma_mpt_create": (_I, [_V, _ip, _I, _I, _I, _dp, _I, _U64]),
    "carma_mpt_start": (_I, [_V, _dp]),
    "carma_mpt_set_chains": (_I, [_V, _dp, _dp]),
    "carma_mpt_get_chains": (_I, [_V, _dp, _dp]),
    "carma_mpt_get_factor": (_I, [_V, _dp]),
    "carma_mpt_set_factor": (_I, [_V, _dp]),
    "carma_mpt_iterate": (_I, [_V, _L, _I]),
    "carma_mpt_sample": (_I, [_V, _I, _I, _dp, _dp]),
    "carma_mpt_stats": (_I, [_V, _dp, _dp, _I]),
    "carma_mpt_iterations_done": (_L, [_V]),
    "carma_mpt_logdensity": (_I, [_V, _dp, _dp]),
    "carma_mpt_kernel_name": (_I, [_V, _S, _I]),
    "carma_mpt_run": (_I, [_V, _ip, _I, _I, _I, _I, _I, _I, _dp, _U64, _dp, _dp]),
    "carma_comm_unique_id": (_I, [_V]),
    "carma_comm_create": (_V, [_V, _I, _I, _I]),
    "carma_comm_destroy": (None, [_V]),
    "carma_comm_rank": (_I, [_V]),
    "carma_comm_size": (_I, [_V]),
}
EXPORTS = list(SIGNATURES)
# (the switches tune_reset puts back; carma_tune_set knows further keys, "MBAND_SMOOTH_CHUNK_ROWS" of BandsContext.smooth and
# "MBANDSET_SMOOTH_CHUNK_WAVES" of BandsSetContext.smooth among them, which a caller moves and resets itself)
TUNE_SWITCHES = ("WIN_ROWS", "WIN2_EVALS", "PT_ROW_WIN", "CSIM_CHUNK_PATHS", "SMOOTH_CHUNK_MODELS")


class CarmaError(RuntimeError):
    """Boost.Python turned C++ exceptions into RuntimeError; so do we."""


class CarmaDeviceError(CarmaError):
    pass


def _share_with_torch(libname):
    """One process, ONE HIP runtime.  The PyTorch wheel bundles its own libamdhip64.so (soname libamdhip64.so.7, like
    the system's); whichever copy is mapped first serves every later request for that soname, but `import torch` asks
    for it by file name and would map a SECOND runtime if this library had already pulled in /opt/rocm's.  Two runtimes
    in one process cannot share streams or device pointers (the `_dev` entry points take torch's) and cooperative
    launches fail outright (measured: hipErrorUnknown).  So when PyTorch is installed and not yet imported, its copy of
    `libname` is mapped first -- without importing torch.  The same for RCCL (bound by the library at run time as
    librccl.so.1), also when torch is imported already: its copy -- and the HIP runtime it was built against -- is the
    one carma_comm_* finds.  CARMA_HIP_RUNTIME=system keeps the system's libraries."""
    if os.environ.get("CARMA_HIP_RUNTIME") == "system" or (libname == "libamdhip64.so" and "torch" in sys.modules):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", libname)
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def build_ids():
    """What is running: {"build_id": sha256 of the shared library that is loaded, "source_id": sha256 over the sources it is
    built from (csrc/, include/, build.sh; None when the sources are not beside the library)}.  Profile records carry
    these so that counters measured on one build are never attributed to another (bench.py, tools/summarize_prof.py)."""
    import hashlib
    out = {"build_id": None, "source_id": None}
    try:
        with open(LIB_PATH, "rb") as f:
            out["build_id"] = hashlib.sha256(f.read()).hexdigest()[:16]
    except OSError:
        pass
    root = os.path.dirname(_HERE)
    files = []
    for sub in ("carma_pack_amd/csrc", "include"):
        dd = os.path.join(root, sub)
        if os.path.isdir(dd):
            files += [os.path.join(dd, f) for f in sorted(os.listdir(dd)) if f.endswith((".h", ".hip", ".hpp", ".cpp"))]
    bs = os.path.join(root, "build.sh")
    if files and os.path.exists(bs):
        h = hashlib.sha256()
        for f in files + [bs]:
            h.update(os.path.relpath(f, root).encode())
            with open(f, "rb") as fh:
                h.update(fh.read())
        out["source_id"] = h.hexdigest()[:16]
    return out


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "carma_pack_amd: %s not found -- build it with ./build.sh (or __graft_entry__.build()); "
            "there is no CPU fallback" % LIB_PATH)
    _share_with_torch("libamdhip64.so")
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    return L


lib = _load()


def tune_set(name, value):
    check(lib.carma_tune_set(str(name).encode(), -2 ** 63 if value is None else int(value)), "carma_tune_set")


tune_set.__doc__ = """Move a launch-shape switch (%s: carma_tune_set; measurements and parity tests).
    value None: back to the library's default.""" % ", ".join('"%s"' % s for s in TUNE_SWITCHES)


def tune_reset():
    """Every switch back to what the environment said when the library read it (CARMA_TUNE_<name>), or to the default."""
    for name in TUNE_SWITCHES:
        e = os.environ.get("CARMA_TUNE_" + name)
        tune_set(name, None if e is None else int(e))


def last_error():
    return lib.carma_last_error().decode()


def check(rc, what):
    if rc == CARMA_OK:
        return
    msg = "%s failed (%d): %s" % (what, rc, last_error())
    if rc == CARMA_ENODEV:
        raise CarmaDeviceError(msg)
    if rc == CARMA_EINVAL:
        raise ValueError(msg)
    raise CarmaError(msg)


def default_device():
    """One process per GPU: LOCAL_RANK picks the device when launched by torch.distributed.run."""
    n = lib.carma_device_count()
    lr = int(os.environ.get("LOCAL_RANK", "0"))
    return lr % n if n > 0 else 0


# ---- marshalling helpers: what every wrapper does to its arguments, once -------------------------
_SINGULAR = "KalmanFilterp: singular eigenvector matrix (solve failed)"


def as_f64(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def ptr(a):
    return a.ctypes.data_as(_dp)


def _optr(a):
    """double* of an optional array: None -> NULL."""
    return None if a is None else a.ctypes.data_as(_dp)


def _iptr(a):
    return a.ctypes.data_as(_ip)


def _lptr(a):
    return a.ctypes.data_as(_lp)


def _dev(device):
    return default_device() if device is None else int(device)


def _seed(seed):
    return C.c_uint64(int(seed) & (2 ** 64 - 1))


def _reim(z):
    """Complex roots [...] -> float64 [..., 2] (re, im), as every entry point takes them; a single root counts as [1]."""
    z = np.atleast_1d(z)
    return as_f64(np.stack([z.real, z.imag], axis=-1))


def _singular(rc, msg):
    """rc == 1 is the library's "repeated AR root" answer of the single-model calls."""
    if rc == 1:
        raise CarmaError(msg)


def _created(h, what, exc=None):
    """The handle a create function returned, or its NULL as the exception (exc None: by the library's message)."""
    if not h:
        msg = "%s failed: %s" % (what, last_error())
        raise (exc or (CarmaDeviceError if "no HIP device" in msg else ValueError))(msg)
    return h


def _default_max_stdev(y):
    # default of the CARMA_Base ctor: 10*sqrt(arma::var(y)) (sample variance, carpack.hpp:71)
    return 10.0 * np.sqrt(np.var(y, ddof=1)) if y.size > 1 else 0.0


def _offsets(sizes):
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    off[1:] = np.cumsum(sizes)
    return off


def _split(a, off):
    return [a[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def _concat_series(series, owner, noun):
    """A list of (t, y, yerr) -> (the y of each, offsets [S + 1], t, y, yerr back to back): MultiContext's series and
    BandsContext's bands."""
    series = list(series)
    if not series:
        raise ValueError("%s needs at least one %s" % (owner, noun))
    cols = []
    for s, item in enumerate(series):
        if len(item) != 3:
            raise ValueError("%s %d: expected (t, y, yerr)" % (noun, s))
        t, y, e = (as_f64(a).ravel() for a in item)
        if not (t.size == y.size == e.size):
            raise ValueError("%s %d: time, y, yerr must have the same length" % (noun, s))
        cols.append((t, y, e))
    ts, ys, es = zip(*cols)
    return (ys, _offsets([t.size for t in ts])) + tuple(as_f64(np.concatenate(a)) for a in (ts, ys, es))


def _theta_rows(thetas, d):
    """thetas [d] or [B, d] -> ([B, d], whether it was one row)."""
    thetas = as_f64(thetas)
    return thetas.reshape(-1, d), thetas.ndim == 1


def _bounds_lohi(bounds):
    """[(lo, hi)] with None for unbounded -> (lo, hi) float64 arrays with -inf / +inf there, as the optimiser entries take a box."""
    return (np.array([-np.inf if b[0] is None else b[0] for b in bounds], dtype=np.float64),
            np.array([np.inf if b[1] is None else b[1] for b in bounds], dtype=np.float64))


def _which(which, B, n=None, noun=None):
    """which (one index per row, or one for all B rows) -> int32 [B] as the library takes it.  n: every index must lie in
    [0, n), a ValueError that names `noun` otherwise; None: the range is the library's check."""
    w = np.ascontiguousarray(np.broadcast_to(np.asarray(which, dtype=np.int64), (B,)))
    if n is not None and B and (w.min() < 0 or w.max() >= n):
        raise ValueError("%s index out of range [0, %d)" % (noun, n))
    return np.ascontiguousarray(w, dtype=np.int32)


def _times_per_row(times, B):
    """One array of times for all B rows, or one per row -- a list or tuple of arrays, or an array of more than one axis -> a
    list: B times the one, or the caller's entries (whose count _pack_times or the caller checks).  Nothing is converted here."""
    if np.ndim(times if isinstance(times, np.ndarray) else 0) > 1 or (isinstance(times, (list, tuple)) and len(times)
                                                                       and np.ndim(times[0]) > 0):
        return list(times)
    return [times] * B


def _pack_times(times, B, who, noun):
    """A list of B arrays of times -> (the arrays, their offsets [B + 1], all of them back to back).  All empty: one dummy time,
    so that the pointers the library gets are valid; outputs are then sized max(offsets[-1], 1)."""
    times = [as_f64(np.atleast_1d(t)).ravel() for t in times]
    if len(times) != B:
        raise ValueError("%s: times must hold one array per %s (%d), got %d" % (who, noun, B, len(times)))
    toff = _offsets([t.size for t in times])
    return times, toff, as_f64(np.concatenate(times)) if toff[-1] else np.zeros(1)


def _pack_models(who, noun, sigsqr, omega, ma=None):
    """The K models of a batched stateless call -> (K, p, sigsqr [K], roots, ma).  With ma: omega [K][p] complex ->
    roots [K][p][2], ma [K][nma]; without (CAR(1)): omega [K] = 1 / tau -> roots [K]."""
    sig = as_f64(np.atleast_1d(sigsqr))
    if ma is None:
        om = as_f64(np.atleast_1d(omega))
        if om.size != sig.size:
            raise ValueError("%s: sigsqr and omega must describe the same number of %s" % (who, noun))
        return sig.size, 1, sig, om, None
    omega = np.atleast_2d(np.asarray(omega, dtype=complex))
    K, p = omega.shape
    ma = as_f64(np.atleast_2d(ma))
    if ma.shape[0] != K or sig.size != K:
        raise ValueError("%s: sigsqr, omega and ma must describe the same number of %s" % (who, noun))
    return K, p, sig, _reim(omega), ma


def _pack_mu(mu, K, who, noun):
    if mu is None:
        return None
    mu = as_f64(np.atleast_1d(mu)).ravel()
    if mu.size != K:
        raise ValueError("%s: mu must have one entry per %s" % (who, noun))
    return mu


def _mle_x0(x0, d):
    x0 = np.ascontiguousarray(np.atleast_2d(np.asarray(x0, dtype=np.float64)))
    B, dd = x0.shape
    if dd != d:
        raise ValueError("x0 must be [B, %d]" % d)
    return x0, B


def _mle_tail(B, d, maxiter, mem, ftol, gtol, fd_step, ignore_prior):
    """The results (x [B, d], fun, nit, nfev, status [B]) of a carma_*mle_batched* call and the arguments all three end in."""
    out = (np.empty((B, d)), np.empty(B)) + tuple(np.zeros(B, dtype=np.int32) for _ in range(3))
    return out, (int(maxiter), int(mem), float(ftol), float(gtol), float(fd_step), 1 if ignore_prior else 0, ptr(out[0]),
                 ptr(out[1])) + tuple(a.ctypes.data_as(C.c_void_p) for a in out[2:])


def _kernel_name(what, *args):
    """A carma_*_kernel_name call: its arguments, then the buffer and its size."""
    buf = C.create_string_buffer(128)
    check(getattr(lib, what)(*args, buf, 128), what)
    return buf.value.decode()


class _Handle:
    """Owns one handle of the library: `_h`, released once by the class's destroy function."""
    _destroy = None

    def close(self):
        if getattr(self, "_h", None):
            getattr(lib, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h


class _Sampler:
    """The parallel-tempering calls of the four contexts.  `_pt` is the prefix of the C functions, `_pt_lead()` the leading shape
    (..., R, T) that pt_create / pt_run left, `_pt_dim()` the entries of a chain's vector.  Everything from pt_set_chains down
    serves all four: Context (carma_pt_*, chains [R][T] of d entries), MultiContext (carma_mpt_*, [M][R][T] of d), BandsContext
    (carma_bands_pt_*, [R][T] of dx) and BandsSetContext (carma_bandset_pt_*, [M][R][T] of dx).

    The three handle-based lane samplers (all but Context) also share ONE create, start and run -- _pt_create, pt_start, _pt_run --
    as the C side shares one front.  Two class attributes say what a class's C calls look like: `_pt_runs`, the arguments lead
    with a run list (w, M) and every shape with M; `_pt_box`, they carry a band box (lo, hi) behind the seed.  A class keeps its
    public pt_create / pt_run, which name the run list as the class does and hand everything on.  A failed create or run leaves
    no sampler behind (`_pt_shape` None: "call pt_create first").  Context has its own three: its init is a list of values with
    a length, and it has the sharding members."""
    _pt = None
    _pt_runs = _pt_box = False

    def _pt_dim(self):
        """Entries of a chain's vector: d of a series; a context whose chains carry more (BandsContext: dx) says so here."""
        return self.d

    def _pt_lead(self):
        if getattr(self, "_pt_shape", None) is None:
            raise ValueError("call pt_create first")
        return self._pt_shape

    def _pt_call(self, name, *args):
        check(getattr(lib, self._pt + name)(self._h, *args), self._pt + name)

    # ---- create, start and run of the lane samplers: the arguments as the C calls take them ----
    def _runs(self, index):
        """The run list (None without one) and what it puts in front of the C arguments and of every shape."""
        if not self._pt_runs:
            return None, (), ()
        w = np.asarray(index, dtype=np.int64).ravel()
        if w.size < 1:
            raise ValueError("need at least one run")
        w = np.ascontiguousarray(w, dtype=np.int32)
        return w, (_iptr(w), w.size), (int(w.size),)              # (w itself: the caller holds it while the C call reads the pointer)

    def _init(self, init, lead):
        """init of start / run: None, or one vector -- with a run list one row per run."""
        if init is None:
            return None
        a = as_f64(init)
        if a.shape != lead + (self._pt_dim(),):
            raise ValueError(("init must be [%d, %d] (one row per run), got %r" if lead else "init must be [%d], got %r")
                             % (lead + (self._pt_dim(), a.shape)))
        return a

    def _band_box(self, band_box, lead):
        """None, or (lo, hi) [K - 1, 2] each, columns (log a_b, mu_b) -- with a run list [M, K - 1, 2], a box per run, or
        [K - 1, 2] for every run -> the two arrays the C calls take (or None, None); nothing for a sampler without a box."""
        if not self._pt_box:
            return ()
        if band_box is None:
            return None, None
        shape = lead + (self.nbands - 1, 2)
        return tuple(as_f64(np.broadcast_to(as_f64(v), shape) if lead and np.ndim(v) == 2 else as_f64(v).reshape(shape))
                     for v in band_box)

    def _pt_create(self, runs, ntemps, nreplicas, adapt_iters, seed, temperatures, band_box=None):
        w, cargs, lead = self._runs(runs)
        tt = as_f64(temperatures) if temperatures is not None else None
        if tt is not None and tt.size != int(ntemps):
            raise ValueError("temperatures must hold ntemps = %d values" % int(ntemps))
        box = self._band_box(band_box, lead)
        self._pt_shape = None
        self._pt_call("create", *cargs, int(ntemps), int(nreplicas), _optr(tt), int(adapt_iters), _seed(seed),
                      *(_optr(v) for v in box))
        self._pt_shape = lead + (int(nreplicas), int(ntemps))

    def pt_start(self, init=None):
        """Starting values (carma_*pt_start); init: None, or a vector of the chains' entries -- with a run list [M, ...], row j for
        run j -- taken by every chain where its log-density there is finite."""
        a = self._init(init, self._pt_lead()[:1] if self._pt_runs else ())
        self._pt_call("start", _optr(a))

    def _pt_run(self, runs, ntemps, nreplicas, sample_size, burnin, thin, init, seed, band_box=None):
        w, cargs, lead = self._runs(runs)
        a = self._init(init, lead)
        box = self._band_box(band_box, lead)
        head = lead + (int(nreplicas), int(sample_size))
        samples, logposts = np.empty(head + (self._pt_dim(),)), np.empty(head)
        self._pt_shape = None
        self._pt_call("run", *cargs, int(ntemps), int(nreplicas), int(sample_size), int(burnin), int(thin), _optr(a), _seed(seed),
                      *(_optr(v) for v in box), ptr(samples), ptr(logposts))
        self._pt_shape = lead + (int(nreplicas), int(ntemps))
        return samples, logposts

    def pt_set_chains(self, theta, logpost=None):
        lead = self._pt_lead()
        theta = as_f64(theta).reshape(lead + (self._pt_dim(),))
        lp = as_f64(logpost).reshape(lead) if logpost is not None else None
        self._pt_call("set_chains", ptr(theta), _optr(lp))

    def pt_get_chains(self):
        lead = self._pt_lead()
        theta, lp = np.empty(lead + (self._pt_dim(),)), np.empty(lead)
        self._pt_call("get_chains", ptr(theta), ptr(lp))
        return theta, lp

    def pt_get_factor(self):
        """chol_factor_ of every chain, [...][R][T][d][d] (upper triangular; src/steps.cpp:32)."""
        chol = np.empty(self._pt_lead() + (self._pt_dim(), self._pt_dim()))
        self._pt_call("get_factor", ptr(chol))
        return chol

    def pt_set_factor(self, chol):
        chol = as_f64(chol).reshape(self._pt_lead() + (self._pt_dim(), self._pt_dim()))
        self._pt_call("set_factor", ptr(chol))

    def pt_iterate(self, niter, do_exchange=True):
        self._pt_call("iterate", int(niter), int(bool(do_exchange)))

    def pt_sample(self, nsamples, thin=1):
        """(samples [...][R][nsamples][d], logposts [...][R][nsamples]) of the coldest chains."""
        head = self._pt_lead()[:-1] + (int(nsamples),)
        samples, logposts = np.empty(head + (self._pt_dim(),)), np.empty(head)
        self._pt_call("sample", int(nsamples), int(thin), ptr(samples), ptr(logposts))
        return samples, logposts

    def pt_stats(self, reset=False):
        lead = self._pt_lead()
        acc, swp = np.empty(lead), np.empty(lead)
        self._pt_call("stats", ptr(acc), ptr(swp), int(bool(reset)))
        return acc, swp

    def pt_iterations_done(self):
        return getattr(lib, self._pt + "iterations_done")(self._h)

    # the handle-based lane samplers (carma_mpt_*, carma_bands_pt_*, carma_bandset_pt_*) only
    def pt_logdensity(self, theta):
        """Log-densities of chain states [...][R][T][dim], each as its chain's run has it (its series or object, its band box),
        through the sampler's own log-density kernel."""
        lead = self._pt_lead()
        theta = as_f64(theta).reshape(lead + (self._pt_dim(),))
        out = np.empty(lead)
        self._pt_call("logdensity", ptr(theta), ptr(out))
        return out

    def pt_kernel_name(self):
        return _kernel_name(self._pt + "kernel_name", self._h)


class Context(_Handle, _Sampler):
    """Owns one carma_ctx (series resident in HBM + prior bounds)."""
    _destroy, _pt = "carma_ctx_destroy", "carma_pt_"

    def __init__(self, time, y, yerr, p, q=0, max_stdev=None, device=None):
        time, y, yerr = as_f64(time), as_f64(y), as_f64(yerr)
        if not (time.size == y.size == yerr.size):
            raise ValueError("time, y, yerr must have the same length")
        if max_stdev is None:
            max_stdev = _default_max_stdev(y)
        self.device = _dev(device)
        self._h = _created(lib.carma_ctx_create(ptr(time), ptr(y), ptr(yerr), time.size, int(p), int(q), float(max_stdev),
                                                self.device), "carma_ctx_create")
        self.p, self.q = int(p), int(q)
        self.n = lib.carma_ctx_n(self._h)
        self.d = lib.carma_ctx_dim(self._h)

    def data(self):
        t, y, e = np.empty(self.n), np.empty(self.n), np.empty(self.n)
        check(lib.carma_ctx_get_data(self._h, ptr(t), ptr(y), ptr(e)), "carma_ctx_get_data")
        return t, y, e

    def prior(self):
        out = np.empty(3)
        check(lib.carma_ctx_get_prior(self._h, ptr(out)), "carma_ctx_get_prior")
        return tuple(out)

    def set_prior(self, max_stdev):
        check(lib.carma_ctx_set_prior(self._h, float(max_stdev)), "carma_ctx_set_prior")

    def logdensity(self, thetas, ignore_prior=False):
        thetas, one = _theta_rows(thetas, self.d)
        out = np.empty(thetas.shape[0])
        check(lib.carma_logdensity_batch(self._h, ptr(thetas), thetas.shape[0], int(bool(ignore_prior)), ptr(out)),
              "carma_logdensity_batch")
        return float(out[0]) if one else out

    def logdensity_dev(self, d_theta_ptr, B, d_out_ptr, ignore_prior=False, stream=0):
        """Enqueue on `stream` (a hipStream_t as int); pointers are device addresses."""
        check(lib.carma_logdensity_batch_dev(self._h, C.c_void_p(d_theta_ptr), int(B), int(bool(ignore_prior)),
                                             C.c_void_p(d_out_ptr), C.c_void_p(stream)),
              "carma_logdensity_batch_dev")

    def kernel_name(self, B):
        """Name of the kernel a launch of B evaluations takes (carma_logdensity_kernel_name)."""
        return _kernel_name("carma_logdensity_kernel_name", self._h, int(B))

    def mle_batched(self, x0, bounds, maxiter=2000, mem=8, ftol=2.220446049250313e-09, gtol=1e-5, fd_step=1e-6,
                    ignore_prior=True):
        """carma_mle_batched: lock-step bounded L-BFGS from every row of x0 on -LogDensity, host loop in the library.
        bounds = [(lo, hi)] with None for unbounded.  Returns (x [B, d], fun [B], nit [B], nfev [B], status [B])."""
        x0, B = _mle_x0(x0, self.d)
        lo, hi = _bounds_lohi(bounds)
        out, tail = _mle_tail(B, self.d, maxiter, mem, ftol, gtol, fd_step, ignore_prior)
        check(lib.carma_mle_batched(self._h, ptr(x0), B, ptr(lo), ptr(hi), *tail), "carma_mle_batched")
        return out

    def logprior(self, theta):
        theta = as_f64(theta)
        return lib.carma_logprior(self._h, ptr(theta))

    # ---- parallel-tempering sampler (RunCarmaSampler / RunCar1Sampler on the GPU); the rest is _Sampler's ----
    def _pt_lead(self):
        return self._pt_shape

    @staticmethod
    def _init_values(init):
        a = as_f64(init) if init is not None and len(init) else None
        return _optr(a), 0 if a is None else a.size

    def pt_run(self, ntemps, nreplicas, sample_size, burnin, thin=1, init=None, seed=0):
        """Whole Sampler::Run; returns (samples[R][S][d], logposts[R][S]) of the coldest chains."""
        samples = np.empty((nreplicas, sample_size, self.d))
        logposts = np.empty((nreplicas, sample_size))
        check(lib.carma_pt_run(self._h, int(ntemps), int(nreplicas), int(sample_size), int(burnin), int(thin),
                               *self._init_values(init), _seed(seed), ptr(samples), ptr(logposts)), "carma_pt_run")
        self._pt_shape = (int(nreplicas), int(ntemps))
        return samples, logposts

    def pt_create(self, ntemps, nreplicas, adapt_iters, seed=0, temperatures=None):
        tt = as_f64(temperatures) if temperatures is not None else None
        check(lib.carma_pt_create(self._h, int(ntemps), int(nreplicas), _optr(tt), int(adapt_iters), _seed(seed)),
              "carma_pt_create")
        self._pt_shape = (int(nreplicas), int(ntemps))

    def pt_shard(self, ntemps_global, slot0, replica0):
        check(lib.carma_pt_shard(self._h, int(ntemps_global), int(slot0), int(replica0)), "carma_pt_shard")
        self._pt_slot0 = int(slot0)

    def pt_bind_state(self, d_theta_ptr, d_logpost_ptr):
        check(lib.carma_pt_bind_state(self._h, C.c_void_p(d_theta_ptr), C.c_void_p(d_logpost_ptr)),
              "carma_pt_bind_state")

    def pt_start(self, init=None):
        check(lib.carma_pt_start(self._h, *self._init_values(init)), "carma_pt_start")

    def pt_debug_draws(self, replica, temperature, iteration):
        """(z[d], u_accept, u_swap): the variates chain (replica, temperature) uses at `iteration`, from the device's own
        generator (carma_pt_debug_draws)."""
        z, ua, us = np.empty(self.d), np.empty(1), np.empty(1)
        check(lib.carma_pt_debug_draws(self._h, int(replica), int(temperature), int(iteration), ptr(z), ptr(ua), ptr(us)),
              "carma_pt_debug_draws")
        return z, float(ua[0]), float(us[0])

    def pt_kernel(self):
        """"row" (k_pt_row), "ladder" (k_pt) or "lane" (k_pt_lane, large ensembles): the sampler kernel this context is on
        (carma_pt_kernel_in_use)."""
        return {1: "row", 2: "lane"}.get(lib.carma_pt_kernel_in_use(self._h), "ladder")

    @staticmethod
    def pt_row_pipeline():
        """Recursion of the process's last k_pt_row launch: "one-datum", "window", "two-sided" (carma_pt_row_pipeline); None before it."""
        return {0: "one-datum", 1: "window", 2: "two-sided"}.get(lib.carma_pt_row_pipeline())

    def pt_boundary_stats(self):
        """(proposed, accepted) swaps across this block's boundaries (carma_pt_iterate_sharded)."""
        a, b = C.c_ulonglong(0), C.c_ulonglong(0)
        check(lib.carma_pt_boundary_stats(self._h, C.byref(a), C.byref(b)), "carma_pt_boundary_stats")
        return a.value, b.value

    def pt_boundary_check(self):
        """1: the last sharded call's boundary self-check agreed; -1: it differed; 0: none yet."""
        return int(lib.carma_pt_boundary_check(self._h))

    def pt_sweep(self):
        """The swap sweep inside this block for the iteration just run with do_exchange=False (carma_pt_sweep)."""
        check(lib.carma_pt_sweep(self._h), "carma_pt_sweep")


class Comm(_Handle):
    """RCCL communicator owned by libcarma_mi355.so (carma_comm_*): one rank per process / GPU.

    ``Comm.unique_id()`` on rank 0 -> 128 bytes to broadcast with the host program's own bootstrap -> every rank
    ``Comm(id, nranks, rank, device)`` (collective)."""
    _destroy = "carma_comm_destroy"

    @staticmethod
    def unique_id():
        _share_with_torch("librccl.so")
        buf = C.create_string_buffer(128)
        check(lib.carma_comm_unique_id(buf), "carma_comm_unique_id")
        return buf.raw

    def __init__(self, unique_id, nranks, rank, device=None):
        _share_with_torch("librccl.so")
        self.device = _dev(device)
        self._id = C.create_string_buffer(bytes(unique_id), 128)
        self._h = _created(lib.carma_comm_create(self._id, int(nranks), int(rank), self.device), "carma_comm_create", CarmaError)
        self.rank, self.size = int(rank), int(nranks)

    @classmethod
    def from_torch(cls, dist, device=None):
        """Bootstrap over an initialised torch.distributed process group (any backend)."""
        rank, world = dist.get_rank(), dist.get_world_size()
        box = [cls.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        return cls(box[0], world, rank, device)


def _sharded(contexts, comm):
    """The leading arguments of the sharded sampler calls: the handles of this process's ladder blocks and their count;
    and the communicator's handle, which follows the call's own counts."""
    return (C.c_void_p * len(contexts))(*[c.handle for c in contexts]), len(contexts), comm._h if comm is not None else None


def pt_iterate_sharded(contexts, niter, comm=None):
    """carma_pt_iterate_sharded: `contexts` = this process's consecutive ladder blocks (normally one)."""
    arr, nctx, ch = _sharded(contexts, comm)
    check(lib.carma_pt_iterate_sharded(arr, nctx, int(niter), ch), "carma_pt_iterate_sharded")


def pt_sample_sharded(contexts, nsamples, thin=1, comm=None):
    """carma_pt_sample_sharded: returns (samples[R][nsamples][d], logposts[R][nsamples]) on the process that owns
    temperature 0, (None, None) elsewhere."""
    arr, nctx, ch = _sharded(contexts, comm)
    c0 = contexts[0]
    owner = getattr(c0, "_pt_slot0", 0) == 0
    R = c0._pt_shape[0]
    samples = np.empty((R, int(nsamples), c0.d)) if owner else None
    logposts = np.empty((R, int(nsamples))) if owner else None
    check(lib.carma_pt_sample_sharded(arr, nctx, int(nsamples), int(thin), ch, _optr(samples), _optr(logposts)),
          "carma_pt_sample_sharded")
    return samples, logposts


class KalmanHandle(_Handle):
    """carma_kf: a KalmanFilter1 / KalmanFilterp object whose series and model stay resident in HBM; Filter and any
    number of (batched) Predict calls only launch and copy results back."""
    _destroy = "carma_kf_destroy"

    def __init__(self, time, y, yerr, sigsqr, omega, ma=None, device=None):
        time, y, yerr = as_f64(time), as_f64(y), as_f64(yerr)
        dev = _dev(device)
        if ma is None:                                   # CAR(1): omega is the real rate 1 / tau
            h = lib.carma_kf_create_car1(ptr(time), ptr(y), ptr(yerr), time.size, float(sigsqr), float(omega), dev)
        else:
            omega = np.asarray(omega, dtype=complex)
            om, ma = _reim(omega), as_f64(ma)
            h = lib.carma_kf_create_carma(ptr(time), ptr(y), ptr(yerr), time.size, omega.size, float(sigsqr), ptr(om),
                                          ptr(ma), ma.size, dev)
        self._h = _created(h, "carma_kf_create")
        self.n = lib.carma_kf_n(self._h)

    def filter(self):
        mean, var = np.empty(self.n), np.empty(self.n)
        rc = lib.carma_kf_filter(self._h, ptr(mean), ptr(var))
        _singular(rc, _SINGULAR)
        check(rc, "carma_kf_filter")
        return mean, var

    def predict(self, tpred):
        tp = as_f64(np.atleast_1d(tpred))
        pm, pv = np.empty(tp.size), np.empty(tp.size)
        rc = lib.carma_kf_predict(self._h, ptr(tp), tp.size, ptr(pm), ptr(pv))
        _singular(rc, _SINGULAR)
        check(rc, "carma_kf_predict")
        return pm, pv


def kfilter_carma(time, y, yerr, sigsqr, omega, ma, device=None):
    time, y, yerr = as_f64(time), as_f64(y), as_f64(yerr)
    omega = np.asarray(omega, dtype=complex)
    om, ma = _reim(omega), as_f64(ma)
    mean, var = np.empty(time.size), np.empty(time.size)
    nout = C.c_int(0)
    rc = lib.carma_kfilter_carma(ptr(time), ptr(y), ptr(yerr), time.size, omega.size, float(sigsqr), ptr(om), ptr(ma),
                                 ma.size, ptr(mean), ptr(var), C.byref(nout), _dev(device))
    _singular(rc, _SINGULAR)
    check(rc, "carma_kfilter_carma")
    return mean[:nout.value], var[:nout.value]


def kfilter_carma_batch(time, y, yerr, sigsqr, omega, ma, mu=None, device=None):
    """Filter() of B models on one series in one launch: sigsqr [B], omega [B][p] complex, ma [B][nma], mu [B] or None
    -> (mean [B][n], var [B][n], singular [B] bool).  mu is subtracted from y inside and added back to mean."""
    time, y, yerr = as_f64(time), as_f64(y), as_f64(yerr)
    B, p, sig, om, ma = _pack_models("kfilter_carma_batch", "models", sigsqr, omega, ma)
    mu_ = _pack_mu(mu, B, "kfilter_carma_batch", "model")
    mean, var = np.empty((B, time.size)), np.empty((B, time.size))
    sing = np.zeros(B, dtype=np.int32)
    nout = C.c_int(0)
    rc = lib.carma_kfilter_batch_carma(ptr(time), ptr(y), ptr(yerr), time.size, p, B, ptr(sig), ptr(om), ptr(ma), ma.shape[1],
                                       _optr(mu_), ptr(mean), ptr(var), _iptr(sing), C.byref(nout), _dev(device))
    check(rc, "carma_kfilter_batch_carma")
    m = nout.value
    # (the library writes rows of n_out values back to back)
    mean = mean.reshape(-1)[:B * m].reshape(B, m)
    var = var.reshape(-1)[:B * m].reshape(B, m)
    return mean, var, sing.astype(bool)


class MultiContext(_Handle, _Sampler):
    """Owns one carma_mctx: MANY series of one order (p, q) resident in HBM, evaluated in shared launches.

    series: a list of (t, y, yerr); each is prepared as Context prepares one (sort, dedup, prior bounds).  max_stdev: None
    (10 sqrt(var(y, ddof=1)) per series, as Context), a number for all series, or one value per series."""
    _destroy, _pt, _pt_runs = "carma_mctx_destroy", "carma_mpt_", True

    def __init__(self, series, p, q=0, max_stdev=None, device=None):
        ys, offsets, t_all, y_all, e_all = _concat_series(series, "MultiContext", "series")
        S = len(ys)
        if max_stdev is None:
            ms = np.array([_default_max_stdev(y) for y in ys])
        else:
            ms = np.broadcast_to(as_f64(max_stdev), (S,)).copy()
        self.device = _dev(device)
        self._h = _created(lib.carma_mctx_create(ptr(t_all), ptr(y_all), ptr(e_all), _lptr(offsets), S, int(p), int(q), ptr(ms),
                                                 self.device), "carma_mctx_create")
        self.p, self.q = int(p), int(q)
        self.nseries = lib.carma_mctx_nseries(self._h)
        self.d = lib.carma_mctx_dim(self._h)
        self.n = np.array([lib.carma_mctx_n(self._h, s) for s in range(self.nseries)], dtype=np.int64)

    def data(self, s):
        n = int(self.n[s])
        t, y, e = np.empty(n), np.empty(n), np.empty(n)
        check(lib.carma_mctx_get_data(self._h, int(s), ptr(t), ptr(y), ptr(e)), "carma_mctx_get_data")
        return t, y, e

    def prior(self, s):
        out = np.empty(3)
        check(lib.carma_mctx_get_prior(self._h, int(s), ptr(out)), "carma_mctx_get_prior")
        return tuple(out)

    def logdensity(self, thetas, which, ignore_prior=False):
        """Log-density of thetas[i] on series which[i] (which: one index per row, or one for all), one launch."""
        thetas, one = _theta_rows(thetas, self.d)
        B = thetas.shape[0]
        w = _which(which, B, self.nseries, "series")
        out = np.empty(B)
        check(lib.carma_mlogdensity_batch(self._h, ptr(thetas), _iptr(w), B, int(bool(ignore_prior)), ptr(out)),
              "carma_mlogdensity_batch")
        return float(out[0]) if one else out

    def kernel_name(self):
        return _kernel_name("carma_mlogdensity_kernel_name", self._h)

    def _items(self, which, sigsqr, roots, ma, mu, who):
        """The (series, model) items of kfilter / predict as the library takes them; every shape error is raised here."""
        sig = as_f64(np.atleast_1d(sigsqr)).ravel()
        M = sig.size
        if M < 1:
            raise ValueError("%s: need at least one item" % who)
        w = _which(which, M, self.nseries, "series")
        roots = np.asarray(roots, dtype=complex)
        if self.p == 1:
            roots = roots.reshape(-1)
            if roots.size != M:
                raise ValueError("%s: roots must hold one root (-omega) per item for a CAR(1) context" % who)
            ma_, nma = np.ones((M, 1)), 1
        else:
            roots = np.atleast_2d(roots)
            if roots.shape != (M, self.p):
                raise ValueError("%s: roots must be [%d, %d] (one row of p roots per item)" % (who, M, self.p))
            ma_ = as_f64(np.atleast_2d(ma))
            if ma_.ndim != 2 or ma_.shape[0] != M or not (1 <= ma_.shape[1] <= self.p):
                raise ValueError("%s: ma must be [%d, nma] with 1 <= nma <= %d" % (who, M, self.p))
            nma = ma_.shape[1]
        return M, w, sig, _reim(roots), ma_, nma, _pack_mu(mu, M, who, "item")

    def kfilter(self, which, sigsqr, roots, ma, mu=None):
        """Filter() of M items in one launch (carma_mkfilter): item i is the model (sigsqr[i], roots[i], ma[i]) on series
        which[i].  sigsqr [M], roots [M][p] complex (p = 1: [M], the root -omega), ma [M][nma] (ignored for p = 1), mu [M] or
        None -- subtracted from y inside and added back to the mean.  Returns (means, vars, singular): lists of M arrays, item
        i's of length n[which[i]], and a bool array."""
        M, w, sig, om, ma_, nma, mu_ = self._items(which, sigsqr, roots, ma, mu, "MultiContext.kfilter")
        off = _offsets(self.n[w])
        mean, var = np.empty(off[-1]), np.empty(off[-1])
        sing = np.zeros(M, dtype=np.int32)
        check(lib.carma_mkfilter(self._h, _iptr(w), M, ptr(sig), ptr(om), ptr(ma_), nma, _optr(mu_), ptr(mean), ptr(var), None,
                                 _iptr(sing)), "carma_mkfilter")
        return _split(mean, off), _split(var, off), sing.astype(bool)

    def _at_times(self, what, who, which, sigsqr, roots, ma, times, mu, return_singular):
        """carma_mpredict / carma_msmooth (`what`): M items, item i at times[i]."""
        M, w, sig, om, ma_, nma, mu_ = self._items(which, sigsqr, roots, ma, mu, who)
        times, toff, tp = _pack_times(times, M, who, "item")
        pm, pv = np.empty(max(int(toff[-1]), 1)), np.empty(max(int(toff[-1]), 1))
        sing = np.zeros(M, dtype=np.int32)
        check(getattr(lib, what)(self._h, _iptr(w), M, ptr(sig), ptr(om), ptr(ma_), nma, _optr(mu_), ptr(tp), _lptr(toff), ptr(pm),
                                 ptr(pv), _iptr(sing)), what)
        if return_singular:
            return _split(pm, toff), _split(pv, toff), sing.astype(bool)
        if sing.any():
            raise CarmaError(_SINGULAR + " for item(s) %s" % np.flatnonzero(sing)[:8].tolist())
        return _split(pm, toff), _split(pv, toff)

    def predict(self, which, sigsqr, roots, ma, times, mu=None, return_singular=False):
        """Predict of M items in one launch (carma_mpredict): item i (as in kfilter) at times[i], a list of M arrays (any of
        them may be empty).  Returns (means, vars): lists of M arrays shaped as times[i].  An item with a repeated AR root
        raises CarmaError, as KalmanHandle.predict does -- or, with return_singular, is flagged in a third return value."""
        return self._at_times("carma_mpredict", "MultiContext.predict", which, sigsqr, roots, ma, times, mu, return_singular)

    def smooth(self, which, sigsqr, roots, ma, times, mu=None, return_singular=False):
        """The interpolated light curve of M items in one call (carma_msmooth): arguments and return values as predict, the
        numbers those of predict to rounding -- but from ONE forward and ONE backward pass over an item's series and times
        (O((n + M_i) p^2) per item instead of O(M_i n p^2)): the route for dense curves.  Items that share a series and a list
        of times share waves; an item's outputs have the bits smooth_carma / smooth_car1 gives for it on its series alone."""
        return self._at_times("carma_msmooth", "MultiContext.smooth", which, sigsqr, roots, ma, times, mu, return_singular)

    def mle_batched(self, x0, which, lo, hi, maxiter=2000, mem=8, ftol=2.220446049250313e-09, gtol=1e-5, fd_step=1e-6,
                    ignore_prior=True):
        """carma_mle_batched_ms: Context.mle_batched with start i on series which[i] and its own box lo[i], hi[i] ([B, d],
        non-finite = unbounded; or [d] for every start).  Returns (x [B, d], fun [B], nit [B], nfev [B], status [B])."""
        x0, B = _mle_x0(x0, self.d)
        w = _which(which, B, self.nseries, "series")
        lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float64), x0.shape))
        hi = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.float64), x0.shape))
        out, tail = _mle_tail(B, self.d, maxiter, mem, ftol, gtol, fd_step, ignore_prior)
        check(lib.carma_mle_batched_ms(self._h, ptr(x0), w.ctypes.data_as(C.c_void_p), B, ptr(lo), ptr(hi), *tail),
              "carma_mle_batched_ms")
        return out

    # ---- parallel-tempering sampler over many series (carma_mpt_*); the rest is _Sampler's --------
    def pt_create(self, series, ntemps, nreplicas, adapt_iters, seed=0, temperatures=None):
        """One sampler run (nreplicas ladders of ntemps chains) per entry of `series` (indices into this context, any order,
        repeats allowed), all advancing in the same launches (carma_mpt_create)."""
        self._pt_create(series, ntemps, nreplicas, adapt_iters, seed, temperatures)

    def pt_run(self, series, ntemps, nreplicas, sample_size, burnin, thin=1, init=None, seed=0):
        """Whole Sampler::Run of every run: (samples [M][R][S][d], logposts [M][R][S]) of the coldest chains (carma_mpt_run)."""
        return self._pt_run(series, ntemps, nreplicas, sample_size, burnin, thin, init, seed)


class BandsContext(_Handle, _Sampler):
    """Owns one carma_bands: K bands of ONE process resident in HBM, band b seen as a_b x(t - lag_b) + mu_b.

    bands: a list of (t, y, yerr), band 0 the reference band; lag_bounds: [K - 1] pairs (lo, hi), the box of every lag.  The
    parameter vector is Context's (d entries) followed by (lag_b, log a_b, mu_b) for b = 1 ... K - 1: dx entries.
    The sampler (carma_bands_pt_*): pt_create / pt_start, then _Sampler's calls on chains [R][T] of dx entries."""
    _destroy, _pt, _pt_box = "carma_bands_destroy", "carma_bands_pt_", True

    def __init__(self, bands, p, q=0, lag_bounds=None, max_stdev=None, device=None):
        ys, offsets, t_all, y_all, e_all = _concat_series(bands, "BandsContext", "band")
        K = len(ys)
        lb = np.zeros((0, 2)) if lag_bounds is None else as_f64(lag_bounds).reshape(-1, 2)
        if lb.shape[0] != K - 1:
            raise ValueError("lag_bounds must hold one (lo, hi) pair for each of the %d bands after the first" % (K - 1))
        lo, hi = (as_f64(lb[:, 0]), as_f64(lb[:, 1])) if K > 1 else (None, None)
        if max_stdev is None:
            max_stdev = _default_max_stdev(ys[0])
        self.device = _dev(device)
        self._h = _created(lib.carma_bands_create(ptr(t_all), ptr(y_all), ptr(e_all), _lptr(offsets), K, int(p), int(q),
                                                  _optr(lo), _optr(hi), float(max_stdev), self.device), "carma_bands_create")
        self.p, self.q = int(p), int(q)
        self.nbands = lib.carma_bands_nbands(self._h)
        self.dx = lib.carma_bands_dim(self._h)
        self.d = self.dx - 3 * (self.nbands - 1)
        self.n = np.array([lib.carma_bands_n(self._h, b) for b in range(self.nbands)], dtype=np.int64)
        self.lag_bounds = lb.copy()

    def prior(self):
        out = np.empty(3)
        check(lib.carma_bands_get_prior(self._h, ptr(out)), "carma_bands_get_prior")
        return tuple(out)

    def logdensity(self, thetas, ignore_prior=False):
        thetas, one = _theta_rows(thetas, self.dx)
        out = np.empty(thetas.shape[0])
        check(lib.carma_bands_logdensity_batch(self._h, ptr(thetas), thetas.shape[0], int(bool(ignore_prior)), ptr(out)),
              "carma_bands_logdensity_batch")
        return float(out[0]) if one else out

    def logdensity_dev(self, d_theta_ptr, B, d_out_ptr, ignore_prior=False, stream=0):
        """Enqueue on `stream` (a hipStream_t as int); pointers are device addresses."""
        check(lib.carma_bands_logdensity_batch_dev(self._h, C.c_void_p(d_theta_ptr), int(B), int(bool(ignore_prior)),
                                                   C.c_void_p(d_out_ptr), C.c_void_p(stream)),
              "carma_bands_logdensity_batch_dev")

    def mle_batched(self, x0, lo=None, hi=None, fixed_lag=None, maxiter=2000, mem=8, ftol=2.220446049250313e-09, gtol=1e-5,
                    fd_step=1e-6, ignore_prior=True):
        """carma_bands_mle_batched: lock-step bounded L-BFGS from every row of x0 [B, dx] on -LogDensity.  lo / hi: [dx] (None
        or non-finite = unbounded; lags stay in their boxes).  fixed_lag [B, K - 1]: the lags of start i are held at
        fixed_lag[i] and come back unchanged in x.  Returns (x [B, dx], fun [B], nit [B], nfev [B], status [B])."""
        x0, B = _mle_x0(x0, self.dx)
        lo = np.full(self.dx, -np.inf) if lo is None else as_f64(lo).reshape(self.dx)
        hi = np.full(self.dx, np.inf) if hi is None else as_f64(hi).reshape(self.dx)
        fl = None if fixed_lag is None else as_f64(fixed_lag).reshape(B, self.nbands - 1)
        out, tail = _mle_tail(B, self.dx, maxiter, mem, ftol, gtol, fd_step, ignore_prior)
        check(lib.carma_bands_mle_batched(self._h, ptr(x0), B, ptr(lo), ptr(hi), _optr(fl), *tail), "carma_bands_mle_batched")
        return out

    def smooth(self, thetas, band, times, moments=False):
        """carma_bands_smooth: mean and variance of a_b x(t - lag_b) + mu_b for b = `band` at the observer times `times` [M] (any
        order, repeats allowed) given ALL data of all bands, under every row of thetas [B, dx] -- one row per lane, each lane on
        the merge order ITS lags give, one forward and one backward pass.  The prior is never applied.
        -> (mean [B, M], var [B, M], invalid [B]); a single vector [dx]: (mean [M], var [M], invalid bool).  moments=True:
        (mean, var, band_mean [M], band_var [M], invalid), the moment-matched mixture over the rows that are not invalid.  An
        invalid row (repeated AR root, non-finite lag, scale or offset) is NaN.  The variance is returned as computed."""
        thetas, one = _theta_rows(thetas, self.dx)
        tp = as_f64(np.atleast_1d(times)).ravel()
        B, M = thetas.shape[0], tp.size
        mean, var = np.empty((B, M)), np.empty((B, M))
        bm, bv = (np.empty(M), np.empty(M)) if moments else (None, None)
        inv = np.zeros(B, dtype=np.int32)
        check(lib.carma_bands_smooth(self._h, ptr(thetas), B, int(band), ptr(tp), M, ptr(mean), ptr(var), _optr(bm), _optr(bv),
                                     _iptr(inv)), "carma_bands_smooth")
        inv = inv.astype(bool)
        if one:
            mean, var, inv = mean[0], var[0], bool(inv[0])
        return (mean, var, bm, bv, inv) if moments else (mean, var, inv)

    # ---- parallel-tempering sampler on the extended vector (carma_bands_pt_*); the rest is _Sampler's --------
    def _pt_dim(self):
        return self.dx

    def pt_default_box(self):
        """(lo, hi) [K - 1, 2] each: the default box of (log a_b, mu_b) (carma_bands_pt_default_box)."""
        lo, hi = np.empty((self.nbands - 1, 2)), np.empty((self.nbands - 1, 2))
        check(lib.carma_bands_pt_default_box(self._h, ptr(lo), ptr(hi)), "carma_bands_pt_default_box")
        return lo, hi

    def pt_create(self, ntemps, nreplicas, adapt_iters, seed=0, temperatures=None, band_box=None):
        """nreplicas ladders of ntemps chains on the extended vector (carma_bands_pt_create).  band_box: None (no box) or (lo, hi),
        [K - 1, 2] each for (log a_b, mu_b): outside it a chain's log-density is -inf."""
        self._pt_create(None, ntemps, nreplicas, adapt_iters, seed, temperatures, band_box)

    def pt_run(self, ntemps, nreplicas, sample_size, burnin, thin=1, init=None, seed=0, band_box=None):
        """Whole Sampler::Run: (samples [R][S][dx], logposts [R][S]) of the coldest chains (carma_bands_pt_run)."""
        return self._pt_run(None, ntemps, nreplicas, sample_size, burnin, thin, init, seed, band_box)


class BandsSetContext(_Handle, _Sampler):
    """Owns one carma_bandset: S multi-band objects of the same K bands and order resident in HBM, each prepared as BandsContext
    prepares its one object; a call carries evaluations of any of them (k_logdens_carma_mband_ms, one object per wave).

    objects: a list of S lists of K (t, y, yerr); lag_bounds: [K - 1] pairs (lo, hi) for every object or [S, K - 1] pairs, one
    list per object; max_stdev: None (BandsContext's default per object), one number or [S].  An object that lacks a band
    belongs to another set.
    The sampler (carma_bandset_pt_*): pt_create / pt_start, then _Sampler's calls on chains [M][R][T] of dx entries, run j of
    the M on object objects[j]."""
    _destroy, _pt, _pt_runs, _pt_box = "carma_bandset_destroy", "carma_bandset_pt_", True, True

    def __init__(self, objects, p, q=0, lag_bounds=None, max_stdev=None, device=None):
        objects = [list(o) for o in objects]
        if not objects:
            raise ValueError("BandsSetContext needs at least one object")
        S, K = len(objects), len(objects[0])
        for s, o in enumerate(objects):
            if len(o) != K or K < 1:
                raise ValueError("object %d has %d bands, object 0 has %d: the objects of a set share their bands" % (s, len(o), K))
        ys, offsets, t_all, y_all, e_all = _concat_series([b for o in objects for b in o], "BandsSetContext", "band")
        lb = np.zeros((S, 0, 2)) if lag_bounds is None else as_f64(lag_bounds)
        if lb.size == (K - 1) * 2:
            lb = np.broadcast_to(lb.reshape(1, K - 1, 2), (S, K - 1, 2))
        if lb.size != S * (K - 1) * 2:
            raise ValueError("lag_bounds must hold one (lo, hi) pair for each of the %d bands after the first, for all objects or "
                             "for each of the %d objects" % (K - 1, S))
        lb = as_f64(lb).reshape(S, K - 1, 2)
        lo, hi = (as_f64(lb[:, :, 0]), as_f64(lb[:, :, 1])) if K > 1 else (None, None)
        if max_stdev is None:
            ms = as_f64([_default_max_stdev(ys[s * K]) for s in range(S)])
        else:
            ms = as_f64(np.broadcast_to(as_f64(max_stdev), (S,)))
        self.device = _dev(device)
        self._h = _created(lib.carma_bandset_create(ptr(t_all), ptr(y_all), ptr(e_all), _lptr(offsets), S, K, int(p), int(q),
                                                    _optr(lo), _optr(hi), ptr(ms), self.device), "carma_bandset_create")
        self.p, self.q = int(p), int(q)
        self.nobjects = lib.carma_bandset_nobjects(self._h)
        self.nbands = lib.carma_bandset_nbands(self._h)
        self.dx = lib.carma_bandset_dim(self._h)
        self.d = self.dx - 3 * (self.nbands - 1)
        self.n = np.array([[lib.carma_bandset_n(self._h, s, b) for b in range(K)] for s in range(S)], dtype=np.int64)
        self.lag_bounds = lb.copy()

    def prior(self, s):
        out = np.empty(3)
        check(lib.carma_bandset_get_prior(self._h, int(s), ptr(out)), "carma_bandset_get_prior")
        return tuple(out)

    def logdensity(self, thetas, which, ignore_prior=False, out=None):
        """Log-density of thetas[i] on object which[i], one launch (carma_bandset_logdensity_batch).  out: a float64 array of at
        least B entries to write the results to (the first B)."""
        thetas, one = _theta_rows(thetas, self.dx)
        B = thetas.shape[0]
        w = _which(which, B)
        if out is None:
            out = np.empty(B)
        elif out.dtype != np.float64 or not out.flags.c_contiguous or out.size < B:
            raise ValueError("out must be a contiguous float64 array of at least %d entries" % B)
        check(lib.carma_bandset_logdensity_batch(self._h, ptr(thetas), _iptr(w), B, int(bool(ignore_prior)), ptr(out)),
              "carma_bandset_logdensity_batch")
        return float(out[0]) if one else out.reshape(-1)[:B]

    def kernel_name(self):
        return _kernel_name("carma_bandset_kernel_name", self._h)

    def mle_batched(self, x0, which, lo=None, hi=None, fixed_lag=None, maxiter=2000, mem=8, ftol=2.220446049250313e-09, gtol=1e-5,
                    fd_step=1e-6, ignore_prior=True):
        """carma_bandset_mle_batched: BandsContext.mle_batched with start i on object which[i] and its own box lo[i], hi[i]
        ([B, dx], or [dx] for every start; None or non-finite = unbounded; lags stay in the boxes of their object).  fixed_lag
        [B, K - 1] as BandsContext.mle_batched.  Returns (x [B, dx], fun [B], nit [B], nfev [B], status [B])."""
        x0, B = _mle_x0(x0, self.dx)
        w = _which(which, B)
        lo = np.ascontiguousarray(np.broadcast_to(as_f64(-np.inf if lo is None else lo), x0.shape))
        hi = np.ascontiguousarray(np.broadcast_to(as_f64(np.inf if hi is None else hi), x0.shape))
        fl = None if fixed_lag is None else as_f64(fixed_lag).reshape(B, self.nbands - 1)
        out, tail = _mle_tail(B, self.dx, maxiter, mem, ftol, gtol, fd_step, ignore_prior)
        check(lib.carma_bandset_mle_batched(self._h, ptr(x0), w.ctypes.data_as(C.c_void_p), B, ptr(lo), ptr(hi), _optr(fl), *tail),
              "carma_bandset_mle_batched")
        return out

    def smooth(self, thetas, which, band, times, return_invalid=False):
        """carma_bandset_smooth: BandsContext.smooth of B rows on any objects of the set in ONE call: row i is the curve of band
        band[i] of object which[i] under thetas[i] ([B, dx]) at the observer times times[i] (any order, repeats allowed, at
        least one).  which, band: one index per row, or one for all rows; times: a list of B arrays, or one array for all rows.
        Returns (means, vars): lists of B arrays shaped as times[i] -- a row has the bits BandsContext.smooth gives it on a
        context of its object alone.  An invalid row (repeated AR root, non-finite lag, scale or offset) is NaN and raises
        CarmaError -- or, with return_invalid, is flagged in a third return value, a bool array [B]."""
        thetas, _ = _theta_rows(thetas, self.dx)
        B = thetas.shape[0]
        w, bo = _which(which, B), _which(band, B)
        times, toff, tp = _pack_times(_times_per_row(times, B), B, "BandsSetContext.smooth", "row")
        mean, var = np.empty(max(int(toff[-1]), 1)), np.empty(max(int(toff[-1]), 1))
        inv = np.zeros(B, dtype=np.int32)
        check(lib.carma_bandset_smooth(self._h, ptr(thetas), _iptr(w), _iptr(bo), B, ptr(tp), _lptr(toff), ptr(mean), ptr(var),
                                       _iptr(inv)), "carma_bandset_smooth")
        if return_invalid:
            return _split(mean, toff), _split(var, toff), inv.astype(bool)
        if inv.any():
            raise CarmaError("BandsSetContext.smooth: a repeated AR root or a non-finite lag, scale or offset for row(s) %s"
                             % np.flatnonzero(inv)[:8].tolist())
        return _split(mean, toff), _split(var, toff)

    # ---- parallel-tempering sampler over many objects (carma_bandset_pt_*); the rest is _Sampler's --------
    def _pt_dim(self):
        return self.dx

    def pt_default_box(self, s):
        """(lo, hi) [K - 1, 2] each: the default box of (log a_b, mu_b) of object s (carma_bandset_pt_default_box)."""
        lo, hi = np.empty((self.nbands - 1, 2)), np.empty((self.nbands - 1, 2))
        check(lib.carma_bandset_pt_default_box(self._h, int(s), ptr(lo), ptr(hi)), "carma_bandset_pt_default_box")
        return lo, hi

    def pt_create(self, objects, ntemps, nreplicas, adapt_iters, seed=0, temperatures=None, band_box=None):
        """One sampler run (nreplicas ladders of ntemps chains on the extended vector) per entry of `objects` (indices into this
        set, any order, repeats allowed), all advancing in the same launches (carma_bandset_pt_create).  band_box: None (no box)
        or (lo, hi), [M, K - 1, 2] each -- a box per run -- or [K - 1, 2] each for every run."""
        self._pt_create(objects, ntemps, nreplicas, adapt_iters, seed, temperatures, band_box)

    def pt_run(self, objects, ntemps, nreplicas, sample_size, burnin, thin=1, init=None, seed=0, band_box=None):
        """Whole Sampler::Run of every run: (samples [M][R][S][dx], logposts [M][R][S]) of the coldest chains
        (carma_bandset_pt_run)."""
        return self._pt_run(objects, ntemps, nreplicas, sample_size, burnin, thin, init, seed, band_box)


def kfilter_car1(time, y, yerr, sigsqr, omega, device=None):
    time, y, yerr = as_f64(time), as_f64(y), as_f64(yerr)
    mean, var = np.empty(time.size), np.empty(time.size)
    nout = C.c_int(0)
    rc = lib.carma_kfilter_car1(ptr(time), ptr(y), ptr(yerr), time.size, float(sigsqr), float(omega), ptr(mean),
                                ptr(var), C.byref(nout), _dev(device))
    check(rc, "carma_kfilter_car1")
    return mean[:nout.value], var[:nout.value]


def predict_carma(time, y, yerr, sigsqr, omega, ma, tpred, device=None):
    """KalmanFilterp::Predict for all `tpred` in one launch -> (mean[M], var[M])."""
    time, y, yerr = as_f64(time), as_f64(y), as_f64(yerr)
    omega = np.asarray(omega, dtype=complex)
    om, ma = _reim(omega), as_f64(ma)
    tp = as_f64(np.atleast_1d(tpred))
    pm, pv = np.empty(tp.size), np.empty(tp.size)
    rc = lib.carma_predict_carma(ptr(time), ptr(y), ptr(yerr), time.size, omega.size, float(sigsqr), ptr(om), ptr(ma),
                                 ma.size, ptr(tp), tp.size, ptr(pm), ptr(pv), _dev(device))
    _singular(rc, _SINGULAR)
    check(rc, "carma_predict_carma")
    return pm, pv


def predict_car1(time, y, yerr, sigsqr, omega, tpred, device=None):
    time, y, yerr = as_f64(time), as_f64(y), as_f64(yerr)
    tp = as_f64(np.atleast_1d(tpred))
    pm, pv = np.empty(tp.size), np.empty(tp.size)
    check(lib.carma_predict_car1(ptr(time), ptr(y), ptr(yerr), time.size, float(sigsqr), float(omega), ptr(tp), tp.size,
                                 ptr(pm), ptr(pv), _dev(device)), "carma_predict_car1")
    return pm, pv


def simulate_carma(time, sigsqr, omega, ma, npaths=1, seed=0, device=None):
    """carma_process for `npaths` paths in one launch -> [npaths][n] at the sorted times (carma_simulate_carma)."""
    time = as_f64(np.sort(np.asarray(time, dtype=float)))
    omega = np.asarray(omega, dtype=complex)
    om, ma = _reim(omega), as_f64(ma)
    out = np.empty((int(npaths), time.size))
    rc = lib.carma_simulate_carma(ptr(time), time.size, omega.size, float(sigsqr), ptr(om), ptr(ma), ma.size, int(npaths),
                                  _seed(seed), ptr(out), _dev(device))
    _singular(rc, "carma_process: repeated AR root (singular eigenvector matrix)")
    check(rc, "carma_simulate_carma")
    return out


def simulate_car1(time, sigsqr, omega, npaths=1, seed=0, device=None):
    time = as_f64(np.sort(np.asarray(time, dtype=float)))
    out = np.empty((int(npaths), time.size))
    check(lib.carma_simulate_car1(ptr(time), time.size, float(sigsqr), float(omega), int(npaths), _seed(seed), ptr(out),
                                  _dev(device)), "carma_simulate_car1")
    return out


def merged_times(time, tsim):
    """The grid the conditional simulation draws its unconditional paths on: the series' distinct times (sorted) followed by
    the sorted `tsim`, in a stable ascending sort -- a requested time equal to a datum comes behind it.
    -> (grid [n + M], position of every datum [n], position of every tsim entry in the caller's order [M])."""
    ts = np.sort(as_f64(np.ravel(time)), kind="stable")
    ts = ts[np.r_[True, np.diff(ts) != 0]]
    tsim = as_f64(np.atleast_1d(tsim))
    perm = np.argsort(tsim, kind="stable")
    cat = np.concatenate([ts, tsim[perm]])
    order = np.argsort(cat, kind="stable")
    inv = np.empty(order.size, dtype=int)
    inv[order] = np.arange(order.size)
    spos = np.empty(tsim.size, dtype=int)
    spos[perm] = inv[ts.size:]
    return cat[order], inv[:ts.size], spos


def _simulate_cond(call, what, time, y, yerr, K, model_args, mu, tsim, seed, path0, return_parts, return_singular, device):
    time, y, yerr = as_f64(time), as_f64(y), as_f64(yerr)
    tp = as_f64(np.atleast_1d(tsim))
    mu_ = _pack_mu(mu, K, what, "path")
    n, M = time.size, tp.size
    out = np.empty((K, max(M, 1)))
    unc = np.empty((K, n + M)) if return_parts else None
    noi = np.empty((K, n)) if return_parts else None
    sing = np.zeros(K, dtype=np.int32)
    nout = C.c_int(0)
    rc = call(ptr(time), ptr(y), ptr(yerr), n, *model_args, _optr(mu_), ptr(tp), M, _seed(seed),
              C.c_uint(int(path0) & 0xffffffff), ptr(out), _optr(unc), _optr(noi), _iptr(sing), C.byref(nout), _dev(device))
    check(rc, what)
    sing = sing.astype(bool)
    if sing.any() and not return_singular:
        raise CarmaError("%s: repeated AR root (singular eigenvector matrix) in path %d" % (what, int(np.argmax(sing))))
    res = (out,)
    if return_parts:
        m = nout.value
        # (the library writes rows of n_out + M and of n_out values back to back)
        res += (unc.reshape(-1)[:K * (m + M)].reshape(K, m + M), noi.reshape(-1)[:K * m].reshape(K, m),
                merged_times(time, tp)[0])
    if return_singular:
        res += (sing,)
    return res[0] if len(res) == 1 else res


def simulate_cond_carma(time, y, yerr, sigsqr, omega, ma, mu, tsim, seed=0, path0=0, return_parts=False,
                        return_singular=False, device=None):
    """K paths of the process at `tsim` CONDITIONAL on the series, path k under its own model (sigsqr[k], omega[k] complex [p],
    ma[k], mu[k]; mu None: 0) and with the generator key (seed, path0 + k), in two launches (carma_simulate_cond_carma)
    -> out [K][M] in the order of tsim.  return_parts: also (uncond [K][n + M], noise [K][n], merged_times [n + M]) -- the
    unconditional paths on the merged grid and the unit normals of the measurement noise, from which simulate_carma and
    predict_carma rebuild every path.  return_singular: also the flags [K] of paths with a repeated AR root (otherwise such
    a path raises)."""
    K, p, sig, om, ma = _pack_models("simulate_cond_carma", "paths", sigsqr, omega, ma)
    return _simulate_cond(lib.carma_simulate_cond_carma, "carma_simulate_cond_carma", time, y, yerr, K,
                          (p, K, ptr(sig), ptr(om), ptr(ma), ma.shape[1]), mu, tsim, seed, path0, return_parts,
                          return_singular, device)


def simulate_cond_car1(time, y, yerr, sigsqr, omega, mu, tsim, seed=0, path0=0, return_parts=False, return_singular=False,
                       device=None):
    """simulate_cond_carma for CAR(1) models: sigsqr [K], omega [K] = 1 / tau (carma_simulate_cond_car1)."""
    K, _, sig, om, _ = _pack_models("simulate_cond_car1", "paths", sigsqr, omega)
    return _simulate_cond(lib.carma_simulate_cond_car1, "carma_simulate_cond_car1", time, y, yerr, K,
                          (K, ptr(sig), ptr(om)), mu, tsim, seed, path0, return_parts, return_singular, device)


def _smooth(call, what, time, y, yerr, K, model_args, mu, tout, band, return_singular, device):
    time, y, yerr = as_f64(time), as_f64(y), as_f64(yerr)
    tp = as_f64(np.atleast_1d(tout))
    mu_ = _pack_mu(mu, K, what, "model")
    if band not in (False, True, "only"):
        raise ValueError("%s: band must be False, True or 'only'" % what)
    M = tp.size
    mean, var = (np.empty((K, M)), np.empty((K, M))) if band != "only" else (None, None)
    bm, bv = (np.empty(M), np.empty(M)) if band else (None, None)
    sing = np.zeros(K, dtype=np.int32)
    nout = C.c_int(0)
    rc = call(ptr(time), ptr(y), ptr(yerr), time.size, *model_args, _optr(mu_), ptr(tp), M, _optr(mean), _optr(var), _optr(bm),
              _optr(bv), _iptr(sing), C.byref(nout), _dev(device))
    check(rc, what)
    sing = sing.astype(bool)
    if sing.any() and not return_singular:
        raise CarmaError("%s: repeated AR root (singular eigenvector matrix) in model %d" % (what, int(np.argmax(sing))))
    return ((mean, var) if band != "only" else ()) + ((bm, bv) if band else ()) + ((sing,) if return_singular else ())


def smooth_carma(time, y, yerr, sigsqr, omega, ma, mu, tout, band=False, return_singular=False, device=None):
    """The interpolated light curve at `tout` under K models at once, in ONE forward and ONE backward pass over the series per
    model (carma_smooth_carma): model k = (sigsqr[k], omega[k] complex [p], ma[k], mu[k]; mu None: 0)
    -> (mean [K][M], var [K][M]) in the order of tout: what predict_carma gives per model, for O((n + M) p^2) instead of
    O(M n p^2).  band=True: also (band_mean [M], band_var [M]), the moment-matched Gaussian mixture over the models that are not
    singular; band="only": just those two (the K x M arrays never leave the device).  return_singular: also the flags [K] of
    models with a repeated AR root (otherwise such a model raises); a flagged model is left out of the band.  The variance is
    returned as computed (a difference: see include/carma_mi355.h), never clipped."""
    K, p, sig, om, ma = _pack_models("smooth_carma", "models", sigsqr, omega, ma)
    return _smooth(lib.carma_smooth_carma, "carma_smooth_carma", time, y, yerr, K, (p, K, ptr(sig), ptr(om), ptr(ma), ma.shape[1]),
                   mu, tout, band, return_singular, device)


def smooth_car1(time, y, yerr, sigsqr, omega, mu, tout, band=False, return_singular=False, device=None):
    """smooth_carma for CAR(1) models: sigsqr [K], omega [K] = 1 / tau (carma_smooth_car1)."""
    K, _, sig, om, _ = _pack_models("smooth_car1", "models", sigsqr, omega)
    return _smooth(lib.carma_smooth_car1, "carma_smooth_car1", time, y, yerr, K, (K, ptr(sig), ptr(om)), mu, tout, band,
                   return_singular, device)


def sigma_noise_batch(ar_roots, ma_coefs, var, device=None):
    """CarmaSample._sigma_noise for all samples in one launch (carma_sigma_noise_batch): ar_roots [ns, p] complex,
    ma_coefs [ns, nma] lowest order first, var [ns] -> sigma [ns]."""
    roots = np.atleast_2d(np.asarray(ar_roots, dtype=complex))
    ns, p = roots.shape
    om = _reim(roots)
    ma = as_f64(np.atleast_2d(np.asarray(ma_coefs, dtype=float)))
    v = as_f64(np.ravel(var))
    if ma.shape[0] != ns or v.size != ns:
        raise ValueError("sigma_noise_batch: one row of roots, MA coefficients and one variance per sample")
    out = np.empty(ns)
    check(lib.carma_sigma_noise_batch(p, ma.shape[1], ptr(om), ptr(ma), ptr(v), ns, ptr(out), _dev(device)),
          "carma_sigma_noise_batch")
    return out


def psd_band(ar_coefs, ma_coefs, sigma, freq, percentiles, return_samples=False, device=None):
    """The power spectrum of every sample on `freq` and np.percentile(..., percentiles) over the samples, on the device
    (carma_psd_band).  ar_coefs [ns, p + 1] highest order first, ma_coefs [ns, nma] lowest first, sigma [ns].
    Returns band [nf, nperc] (and the grid [nf, ns] with return_samples)."""
    ar = as_f64(np.atleast_2d(np.asarray(ar_coefs, dtype=float)))
    ma = as_f64(np.atleast_2d(np.asarray(ma_coefs, dtype=float)))
    sg = as_f64(np.ravel(sigma))
    fr = as_f64(np.ravel(freq))
    pc = as_f64(np.ravel(percentiles))
    ns = ar.shape[0]
    if ma.shape[0] != ns or sg.size != ns:
        raise ValueError("psd_band: one row of AR coefficients, MA coefficients and one sigma per sample")
    band = np.empty((fr.size, pc.size))
    grid = np.empty((fr.size, ns)) if return_samples else None
    check(lib.carma_psd_band(ar.shape[1], ma.shape[1], ptr(ar), ptr(ma), ptr(sg), ns, ptr(fr), fr.size, ptr(pc), pc.size,
                             ptr(band), _optr(grid), _dev(device)), "carma_psd_band")
    return (band, grid) if return_samples else band


def mpsd_fused_max():
    """The largest sample count of a series that carma_mpsd_band serves with its fused kernel (carma_mpsd_fused_max)."""
    return int(lib.carma_mpsd_fused_max())


def mpsd_freq_tile():
    """Frequencies per workgroup of the fused kernel (carma_mpsd_freq_tile)."""
    return int(lib.carma_mpsd_freq_tile())


def mpsd_band(ar_coefs, ma_coefs, sigma, sample_start, freq, percentiles, device=None):
    """psd_band's percentiles for every series of a set in one call (carma_mpsd_band).  ar_coefs [N, p + 1] highest order
    first, ma_coefs [N, nma] lowest first, sigma [N]: the samples of all S series back to back, series s owning the rows
    sample_start[s] ... sample_start[s + 1] - 1 (sample_start [S + 1], from 0, strictly increasing, ending at N).  freq: [nf]
    for every series, or [S, nf] with a grid per series.  percentiles: 1 ... 4 values in [0, 100].  Returns band [S, nf, nperc]."""
    ar = as_f64(np.atleast_2d(np.asarray(ar_coefs, dtype=float)))
    ma = as_f64(np.atleast_2d(np.asarray(ma_coefs, dtype=float)))
    sg = as_f64(np.ravel(sigma))
    pc = as_f64(np.ravel(percentiles))
    st = np.ascontiguousarray(np.ravel(sample_start), dtype=np.int64)
    if ar.ndim != 2 or ma.ndim != 2:
        raise ValueError("mpsd_band: ar_coefs and ma_coefs must be [N, p + 1] and [N, nma]")
    N = ar.shape[0]
    if ma.shape[0] != N or sg.size != N:
        raise ValueError("mpsd_band: one row of AR coefficients, MA coefficients and one sigma per sample")
    if st.size < 2 or st[0] != 0 or st[-1] != N or (np.diff(st) < 1).any():
        raise ValueError("mpsd_band: sample_start must be [S + 1], start at 0, increase strictly and end at N = %d" % N)
    S = st.size - 1
    fr = as_f64(np.asarray(freq, dtype=float))
    if fr.ndim == 1:
        fr = as_f64(np.broadcast_to(fr, (S, fr.size)))
    if fr.ndim != 2 or fr.shape[0] != S or fr.shape[1] < 1:
        raise ValueError("mpsd_band: freq must be [nf] or [%d, nf] with nf >= 1, got %r" % (S, fr.shape))
    if not 1 <= pc.size <= 4:
        raise ValueError("mpsd_band: 1 ... 4 percentiles, got %d" % pc.size)
    band = np.empty((S, fr.shape[1], pc.size))
    check(lib.carma_mpsd_band(ar.shape[1], ma.shape[1], ptr(ar), ptr(ma), ptr(sg), _lptr(st), S, ptr(fr), fr.shape[1], ptr(pc),
                              pc.size, ptr(band), _dev(device)), "carma_mpsd_band")
    return band


def chain_diag_dmax():
    """The widest column count one carma_chain_diag call serves (carma_chain_diag_dmax)."""
    return int(lib.carma_chain_diag_dmax())


def chain_diag_kernel_ms():
    """Device time in ms of the kernels of the last carma_chain_diag call of this process (carma_chain_diag_kernel_ms)."""
    return float(lib.carma_chain_diag_kernel_ms())


def chain_diag(x, rhat=True, device=None):
    """Chain diagnostics of a whole sampled set on the device (carma_chain_diag).  x: [G, R, L, d] -- G groups of R replicas of
    L samples of d columns; [L], [L, d] and [R, L, d] are taken as one column, one chain, one group.  Returns a dict: tau
    (Goodman's acor autocorrelation time), mean, sigma (the standard error of the mean), status (0 OK, 1 SHORT, 2 CONSTANT,
    3 NONFINITE; tau and sigma are NaN unless it is 0), each [G, R, d], and rhat [G, d] (split R-hat over the replicas of a
    group; None with rhat=False).  More than chain_diag_dmax() columns are served in slabs of that many."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[None, None, :, None]
    elif x.ndim == 2:
        x = x[None, None]
    elif x.ndim == 3:
        x = x[None]
    if x.ndim != 4:
        raise ValueError("chain_diag: x must be [G, R, L, d] ([L], [L, d] and [R, L, d] are promoted), got %d axes" % x.ndim)
    if 0 in x.shape:
        raise ValueError("chain_diag: x has an empty axis: %r" % (x.shape,))
    G, R, L, d = x.shape
    dev = _dev(device)
    dmax = chain_diag_dmax()
    out = dict(tau=np.empty((G, R, d)), mean=np.empty((G, R, d)), sigma=np.empty((G, R, d)),
               status=np.empty((G, R, d), dtype=np.int32), rhat=np.empty((G, d)) if rhat else None)
    for c0 in range(0, d, dmax):
        c1 = min(d, c0 + dmax)
        xs = as_f64(x if (c0, c1) == (0, d) else x[..., c0:c1])
        part = [np.empty((G, R, c1 - c0)) for _ in range(3)]
        st = np.empty((G, R, c1 - c0), dtype=np.int32)
        rh = np.empty((G, c1 - c0)) if rhat else None
        check(lib.carma_chain_diag(ptr(xs), G, R, L, c1 - c0, ptr(part[0]), ptr(part[1]), ptr(part[2]), _iptr(st), _optr(rh), dev),
              "carma_chain_diag")
        for k, name in enumerate(("tau", "mean", "sigma")):
            out[name][..., c0:c1] = part[k]
        out["status"][..., c0:c1] = st
        if rhat:
            out["rhat"][:, c0:c1] = rh
    return out


def normalize_roots(omega):
    """AR roots in any order -> conjugate pairs adjacent (negative imaginary part first), real roots last
    (carma_normalize_roots; host arithmetic, no device needed).  ValueError when the set is not closed under conjugation."""
    omega = np.asarray(omega, dtype=complex)
    om = _reim(omega)
    out = np.empty_like(om)
    rc = lib.carma_normalize_roots(omega.size, ptr(om), ptr(out))
    if rc != CARMA_OK:
        raise ValueError("the AR roots must be real or come in complex-conjugate pairs")
    return out[:, 0] + 1j * out[:, 1]
