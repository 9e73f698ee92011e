"""CPU-only tests of the set call for power-spectrum bands (carma_mpsd_band, _lib.mpsd_band,
CarmaModelSet.power_spectrum_band): the symbols exist, and every argument error is reported before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22


def test_library_exports_and_header_declares_the_set_entries():
    import carma_pack_amd._lib as L
    dll = C.CDLL(L.LIB_PATH)
    txt = open(os.path.join(ROOT, "include", "carma_mi355.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("carma_mpsd_band", "carma_mpsd_fused_max"):
        assert hasattr(dll, name), "libcarma_mi355.so does not export %s" % name
        assert re.search(r"\b%s\s*\(" % name, txt), "include/carma_mi355.h does not declare %s" % name
        assert name in L.EXPORTS


def test_fused_limit_holds_a_thousand_samples():
    import carma_pack_amd._lib as L
    assert L.lib.carma_mpsd_fused_max() >= 1024
    assert L.mpsd_fused_max() == L.lib.carma_mpsd_fused_max()
    assert L.mpsd_freq_tile() >= 1


def _call(L, nar=3, nma=1, ar=True, ma=True, sigma=True, start=(0, 2, 5), nseries=2, freq=True, nf=3, perc=(16.0, 50.0), nperc=None,
          band=True):
    N = 5
    a, m, s = np.ones((N, max(nar, 1))), np.ones((N, max(nma, 1))), np.ones(N)
    st = np.asarray(start, dtype=np.int64) if start is not None else None
    f = np.full((max(nseries, 1), max(nf, 1)), 0.1)
    pc = np.asarray(perc, dtype=float)
    out = np.full((max(nseries, 1), max(nf, 1), 4), -777.0)
    rc = L.lib.carma_mpsd_band(nar, nma, L.ptr(a) if ar else None, L.ptr(m) if ma else None, L.ptr(s) if sigma else None,
                               st.ctypes.data_as(C.POINTER(C.c_long)) if st is not None else None, nseries,
                               L.ptr(f) if freq else None, nf, L.ptr(pc) if perc is not None else None,
                               pc.size if nperc is None else nperc, L.ptr(out) if band else None, 0)
    assert (out == -777.0).all()
    return rc


def test_every_argument_error_returns_einval_without_a_device():
    import carma_pack_amd._lib as L
    bad = [dict(ar=False), dict(ma=False), dict(sigma=False), dict(start=None), dict(freq=False), dict(perc=None, nperc=2),
           dict(band=False),
           dict(nar=1), dict(nar=L.PMAX + 2), dict(nma=0), dict(nma=L.PMAX + 1),
           dict(nseries=0), dict(nseries=-1), dict(nf=0),
           dict(start=(1, 2, 5)), dict(start=(0, 2, 2)), dict(start=(0, 3, 2)), dict(start=(0, 0, 5)),
           dict(nperc=0), dict(perc=(1.0, 2.0, 3.0, 4.0, 5.0)),
           dict(perc=(-0.5, 50.0)), dict(perc=(50.0, 100.5)), dict(perc=(np.nan,))]
    for kw in bad:
        assert _call(L, **kw) == EINVAL, kw
        assert "carma_mpsd_band" in L.last_error(), kw
    # a well-formed call gets past the argument checks: without a device it fails for that reason, with one it succeeds
    rc = _call(L) if L.lib.carma_device_count() == 0 else 0
    assert rc in (0, L.CARMA_ENODEV)


def test_binding_raises_on_mismatched_shapes():
    import carma_pack_amd._lib as L
    ar, ma, sg = np.ones((5, 3)), np.ones((5, 1)), np.ones(5)
    ok = dict(ar_coefs=ar, ma_coefs=ma, sigma=sg, sample_start=[0, 2, 5], freq=[0.1, 0.2], percentiles=[16.0, 50.0])
    bad = [dict(ma_coefs=np.ones((4, 1))), dict(sigma=np.ones(6)), dict(sample_start=[0, 2, 4]), dict(sample_start=[1, 2, 5]),
           dict(sample_start=[0, 2, 2, 5]), dict(sample_start=[5]), dict(freq=np.ones((3, 2))), dict(freq=np.ones((2, 0))),
           dict(freq=np.ones((2, 2, 2))), dict(percentiles=[]), dict(percentiles=[1.0, 2.0, 3.0, 4.0, 5.0])]
    for kw in bad:
        with pytest.raises(ValueError):
            L.mpsd_band(**dict(ok, **kw))
    if L.lib.carma_device_count() == 0:                       # the well-formed call reaches the library
        with pytest.raises(L.CarmaDeviceError):
            L.mpsd_band(**ok)


def test_set_band_needs_samples_of_the_right_length():
    import carma_pack_amd as cpa
    t = np.arange(20.0)
    series = [(t, np.sin(t), np.full(20, 0.1)), (t, np.cos(t), np.full(20, 0.1)), (t, np.sin(2 * t), np.full(20, 0.1))]
    mset = cpa.CarmaModelSet(series, p=2, q=1)
    with pytest.raises(ValueError):
        mset.power_spectrum_band()                           # before any run
    with pytest.raises(ValueError):
        mset.power_spectrum_band(samples=[object(), object()])
    with pytest.raises(ValueError):
        mset.power_spectrum_band(samples=[])
