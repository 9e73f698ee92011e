"""CPU-only: argument checks of the multi-series entry points (carma_mctx_*, carma_mlogdensity_batch, carma_mle_batched_ms)
come before any device work, and the Python classes over them (MultiContext, CarmaModelSet) check their inputs and fail
loudly without a GPU."""
import ctypes as C

import numpy as np
import pytest

import carma_pack_amd as cpa
import carmcmc as cm

L = cpa._lib.lib
EINVAL = -22


def _no_gpu():
    if L.carma_device_count() > 0:
        pytest.skip("a GPU is visible")


def _create(t, y, e, offsets, S, p, q, max_stdev=None):
    t, y, e = (np.ascontiguousarray(a, dtype=np.float64) for a in (t, y, e))
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    ms = None if max_stdev is None else np.ascontiguousarray(max_stdev, dtype=np.float64)
    dp = C.POINTER(C.c_double)
    h = L.carma_mctx_create(t.ctypes.data_as(dp), y.ctypes.data_as(dp), e.ctypes.data_as(dp),
                            off.ctypes.data_as(C.POINTER(C.c_long)), S, p, q, None if ms is None else ms.ctypes.data_as(dp), 0)
    return h, cpa._lib.last_error()


def test_mctx_create_argument_errors_before_device_work():
    """Without a GPU, every argument error is reported as such (the device check comes last)."""
    _no_gpu()
    t = np.concatenate([np.arange(10.0), np.arange(5.0)])
    y, e = np.sin(t), np.ones(t.size)
    h, msg = _create(t, y, e, [0, 10, 15], 2, 8, 0)
    assert not h and "1 <= p <= 7" in msg
    h, msg = _create(t, y, e, [0, 10, 15], 2, 3, 3)
    assert not h and "q < p" in msg
    h, msg = _create(t, y, e, [0, 10, 15], 2, 1, 1)
    assert not h and "q < p" in msg
    h, msg = _create(t, y, e, [0, 10, 5], 2, 2, 1)
    assert not h and "non-decreasing" in msg
    h, msg = _create(t, y, e, [0], 0, 2, 1)
    assert not h and "nseries >= 1" in msg
    # a series with one distinct time (after dedup) is named by its index
    t2 = t.copy()
    t2[10:15] = 3.0
    h, msg = _create(t2, y, e, [0, 10, 15], 2, 2, 1)
    assert not h and "series 1 has fewer than 2 distinct times" in msg
    h, msg = _create(t, y, e, [0, 10, 11], 2, 2, 1)
    assert not h and "series 1 has fewer than 2 distinct times" in msg
    # a valid set: only now the device is asked for
    h, msg = _create(t, y, e, [0, 10, 15], 2, 2, 1)
    assert not h and "no HIP device" in msg


def test_null_handles_are_einval():
    x = np.zeros(8)
    vp = x.ctypes.data_as(C.c_void_p)
    ip = np.zeros(2, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    assert L.carma_mctx_nseries(None) == EINVAL
    assert L.carma_mctx_dim(None) == EINVAL
    assert L.carma_mctx_n(None, 0) == EINVAL
    assert L.carma_mctx_get_prior(None, 0, x.ctypes.data_as(C.POINTER(C.c_double))) == EINVAL
    assert L.carma_mlogdensity_batch(None, x.ctypes.data_as(C.POINTER(C.c_double)), ip, 1, 0,
                                     x.ctypes.data_as(C.POINTER(C.c_double))) == EINVAL
    assert L.carma_mle_batched_ms(None, vp, vp, 1, None, None, 10, 8, 1e-9, 1e-5, 1e-6, 1, vp, vp, None, None, None) == EINVAL
    L.carma_mctx_destroy(None)


def test_multicontext_raises_device_error_without_gpu():
    _no_gpu()
    t = np.arange(20.0)
    with pytest.raises(cpa.CarmaDeviceError):
        cpa.MultiContext([(t, np.sin(t), np.ones(20)), (t[:7], np.cos(t[:7]), np.ones(7))], 3, 1)
    with pytest.raises(ValueError):                           # host-side checks first
        cpa.MultiContext([(t, np.sin(t), np.ones(20)), (np.ones(3), np.ones(3), np.ones(3))], 3, 1)
    with pytest.raises(ValueError):
        cpa.MultiContext([], 2, 1)
    with pytest.raises(ValueError):
        cpa.MultiContext([(t, np.sin(t), np.ones(19))], 2, 1)


def test_carma_model_set_input_checks():
    t = np.arange(20.0)
    ok = (t, np.sin(t), np.ones(20))
    with pytest.raises(ValueError):
        cm.CarmaModelSet([])
    with pytest.raises(ValueError):
        cm.CarmaModelSet([ok], p=2, q=2)
    with pytest.raises(ValueError):
        cm.CarmaModelSet([ok, (t, np.sin(t))])
    with pytest.raises(ValueError):
        cm.CarmaModelSet([ok, (t, np.sin(t), np.ones(5))])
    with pytest.raises(ValueError):
        cm.CarmaModelSet([ok, (np.full(4, 2.0), np.ones(4), np.ones(4))])
    ms = cm.CarmaModelSet([ok, (t[::-1], np.cos(t)[::-1], np.ones(20))], p=2, q=1)
    assert ms.nseries == 2 and np.all(np.diff(ms.models[1].time) > 0)
    with pytest.raises(ValueError):                           # starts of the wrong shape, before any device work
        ms.get_mle(2, 1, starts=np.zeros((3, 4, 6)))
    with pytest.raises(ValueError):
        ms.loglik(np.zeros(6), 2)
    with pytest.raises(ValueError):
        ms.choose_order(0)
