"""The recording stand-in for `carma_pack_amd._lib.lib` that the CPU-only call tests share (test_lib_marshalling_cpu.py,
test_models_calls_cpu.py), and the helpers that read and write the arrays behind its pointer arguments.

A FakeLib is a plain Python object: its `carma_*` functions keep their arguments in `calls`, run the function scripted for
their name in `on` (which copies arrays out with `rd`, fills output pointers with `wr` / `fill` and returns a code), and
otherwise return the handle H from a create function, None from a destroy function and 0 from everything else.  No device and
no library call is made."""
import ctypes as C

import numpy as np

H = 0x5000                                                    # the handle every scripted create function returns
CREATORS = ("carma_ctx_create", "carma_mctx_create", "carma_bands_create", "carma_bandset_create", "carma_kf_create_car1",
            "carma_kf_create_carma", "carma_comm_create")
CTYPES = {float: C.c_double, np.int32: C.c_int, np.int64: C.c_long}


def _view(p, shape, dtype=float):
    n = int(np.prod(shape))
    addr = C.cast(p, C.c_void_p).value
    assert addr, "NULL where an array was expected"
    return np.ctypeslib.as_array((CTYPES[dtype] * n).from_address(addr)).reshape(shape)


def rd(p, shape, dtype=float):
    """A copy of the array behind a pointer argument."""
    return _view(p, shape, dtype).copy()


def wr(p, values, dtype=float):
    """Write `values` (any shape, C order) through an output pointer."""
    values = np.asarray(values)
    _view(p, values.shape, dtype)[...] = values


def fill(p, shape, start=0, dtype=float):
    wr(p, np.arange(start, start + int(np.prod(shape))).reshape(shape), dtype)


def val(x):
    """A scalar argument as a Python number, whether it came as one or as a ctypes object; None stays None (NULL)."""
    return x.value if hasattr(x, "value") else x


def null(p):
    return p is None or not C.cast(p, C.c_void_p).value


def setref(ref, v):
    ref._obj.value = v                                         # (the object behind a byref())


class FakeLib:
    def __init__(self):
        self.calls, self.on, self.error = [], {}, b"scripted failure"

    def __getattr__(self, name):
        if not name.startswith("carma_"):
            raise AttributeError(name)

        def fn(*a):
            self.calls.append((name, a))
            if name in self.on:
                return self.on[name](*a)
            if name == "carma_last_error":
                return self.error
            return H if name in CREATORS else None if name.endswith("_destroy") else 0
        return fn

    def args(self, name, k=-1):
        return [a for n, a in self.calls if n == name][k]

    def count(self, name):
        return sum(n == name for n, _ in self.calls)
