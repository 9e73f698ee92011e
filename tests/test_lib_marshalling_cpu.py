"""CPU-only: what every wrapper of carma_pack_amd/_lib.py hands to the C ABI and what it makes of the answer.

`_lib.lib` is replaced by a recording stand-in (a plain Python object): its functions keep the scalar arguments, copy out the
arrays behind pointer arguments at the shapes the test states, write scripted values into output pointers and `byref` integers and
return a scripted code or handle.  Outputs are filled with `arange`, so a wrong reshape or transposition shows.  Shapes: n = 5,
p = 3, q = 1 (d = 6), two series of 3 and 2 data, K = 2 bands, B = M = 3, R = 2, T = 3.  No device and no library call is made."""
import ctypes as C
import gc

import numpy as np
import pytest

import carma_pack_amd._lib as L
from fakelib import H, FakeLib, fill, null, rd, setref, val, wr

N, P, Q, D, R, T = 5, 3, 1, 6, 2, 3
T5, Y5, E5 = np.arange(5.0), np.array([1.0, 3.0, 2.0, 5.0, 4.0]), np.full(5, 0.1)
SERIES = [(T5[:3], Y5[:3], E5[:3]), (T5[3:], Y5[3:], E5[3:])]
ROOTS = np.array([-0.5 + 1j, -0.5 - 1j, -2.0])               # one model; [K][p] models below
ROOTS3 = np.stack([ROOTS, 2 * ROOTS, 3 * ROOTS])
MA3 = np.array([[1.0, 0.5], [1.0, 0.25], [1.0, 0.125]])
SIG3 = np.array([1.0, 2.0, 3.0])
REIM3 = np.stack([ROOTS3.real, ROOTS3.imag], axis=-1)


@pytest.fixture
def fake(monkeypatch):
    f = FakeLib()
    monkeypatch.setattr(L, "lib", f)
    monkeypatch.setenv("CARMA_HIP_RUNTIME", "system")          # Comm maps no library into this process
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    f.on.update(carma_ctx_n=lambda h: N, carma_ctx_dim=lambda h: D, carma_mctx_nseries=lambda h: 2, carma_mctx_dim=lambda h: D,
                carma_mctx_n=lambda h, s: (3, 2)[s], carma_kf_n=lambda h: N)
    yield f
    # an object a traceback still holds is released after the real library is back: it must not hand that one a scripted handle
    for o in gc.get_objects():
        if type(o) in (L.Context, L.MultiContext, L.BandsContext, L.BandsSetContext, L.KalmanHandle, L.Comm) and getattr(o, "_h", None) in (H, H + 8, H + 16):
            o._h = None


def make_ctx(fake, **kw):
    return L.Context(T5, Y5, E5, P, Q, **kw)


def make_mctx(fake, p=P, **kw):
    return L.MultiContext(SERIES, p, Q if p > 1 else 0, **kw)


def make_bands(fake, K=2, **kw):
    fake.on.update(carma_bands_nbands=lambda h: K, carma_bands_dim=lambda h: D + 3 * (K - 1), carma_bands_n=lambda h, b: (3, 2)[b])
    if K == 2:
        kw.setdefault("lag_bounds", [(-1.0, 1.5)])
    return L.BandsContext(SERIES[:K], P, Q, **kw)


# ---- check(), devices, switches -------------------------------------------------------------------
def test_check_maps_codes_to_exceptions(fake):
    L.check(0, "carma_x")
    for rc, exc in ((-19, L.CarmaDeviceError), (-22, ValueError), (-5, L.CarmaError), (-12, L.CarmaError), (3, L.CarmaError)):
        with pytest.raises(exc) as e:
            L.check(rc, "carma_x")
        assert type(e.value) is exc and str(e.value) == "carma_x failed (%d): scripted failure" % rc
    assert L.last_error() == "scripted failure"


def test_default_device_follows_local_rank(fake, monkeypatch):
    assert L.default_device() == 0                             # no device: 0
    fake.on["carma_device_count"] = lambda: 4
    assert L.default_device() == 0
    monkeypatch.setenv("LOCAL_RANK", "6")
    assert L.default_device() == 2
    make_ctx(fake)
    assert val(fake.args("carma_ctx_create")[7]) == 2
    make_ctx(fake, device=np.int64(3))
    assert val(fake.args("carma_ctx_create")[7]) == 3


def test_tune_set_and_reset(fake, monkeypatch):
    L.tune_set("WIN_ROWS", 12)
    L.tune_set("WIN_ROWS", None)
    assert [(a[0], val(a[1])) for n, a in fake.calls] == [(b"WIN_ROWS", 12), (b"WIN_ROWS", -2 ** 63)]
    fake.calls.clear()
    names = ("WIN_ROWS", "WIN2_EVALS", "PT_ROW_WIN", "CSIM_CHUNK_PATHS", "SMOOTH_CHUNK_MODELS")
    for nm in names:
        monkeypatch.delenv("CARMA_TUNE_" + nm, raising=False)
        assert '"%s"' % nm in L.tune_set.__doc__
    monkeypatch.setenv("CARMA_TUNE_PT_ROW_WIN", "7")
    L.tune_reset()
    assert [(a[0].decode(), val(a[1])) for n, a in fake.calls] == [(nm, 7 if nm == "PT_ROW_WIN" else -2 ** 63) for nm in names]
    fake.on["carma_tune_set"] = lambda n, v: -22
    with pytest.raises(ValueError, match=r"carma_tune_set failed \(-22\)"):
        L.tune_set("NOPE", 1)


# ---- handles ----------------------------------------------------------------------------------------
def _kf_car1(fake, **kw):
    return L.KalmanHandle(T5, Y5, E5, 2.0, 0.25, **kw)


def _kf_carma(fake, **kw):
    return L.KalmanHandle(T5, Y5, E5, 2.0, ROOTS, MA3[0], **kw)


def _comm(fake, **kw):
    return L.Comm(b"\x07" * 128, 4, 1, **kw)


MAKERS = [(make_ctx, "carma_ctx_create", "carma_ctx_destroy", "carma_ctx_create failed: ", ValueError),
          (make_mctx, "carma_mctx_create", "carma_mctx_destroy", "carma_mctx_create failed: ", ValueError),
          (make_bands, "carma_bands_create", "carma_bands_destroy", "carma_bands_create failed: ", ValueError),
          (_kf_car1, "carma_kf_create_car1", "carma_kf_destroy", "carma_kf_create failed: ", ValueError),
          (_kf_carma, "carma_kf_create_carma", "carma_kf_destroy", "carma_kf_create failed: ", ValueError),
          (_comm, "carma_comm_create", "carma_comm_destroy", "carma_comm_create failed: ", L.CarmaError)]


@pytest.mark.parametrize("make,create,destroy,prefix,exc", MAKERS, ids=[m[1] for m in MAKERS])
def test_handle_lifetime_and_null_handle(fake, make, create, destroy, prefix, exc):
    obj = make(fake)
    assert obj._h == H and fake.count(create) == 1
    obj.close()
    obj.close()
    assert obj._h is None
    obj.__del__()
    assert fake.count(destroy) == 1 and fake.args(destroy) == (H,)
    fake.on[create] = lambda *a: None                         # NULL
    with pytest.raises(exc) as e:
        make(fake)
    assert type(e.value) is exc and str(e.value) == prefix + "scripted failure"
    fake.error = b"device 3: no HIP device here"
    with pytest.raises(L.CarmaError) as e:
        make(fake)
    assert type(e.value) is (L.CarmaError if create == "carma_comm_create" else L.CarmaDeviceError)
    assert str(e.value) == prefix + "device 3: no HIP device here"
    assert fake.count(destroy) == 1                           # nothing to release after a failed create


def test_context_create_arguments(fake):
    ctx = make_ctx(fake)
    a = fake.args("carma_ctx_create")
    assert [rd(a[i], (N,)).tolist() for i in range(3)] == [T5.tolist(), Y5.tolist(), E5.tolist()]
    assert [val(x) for x in a[3:6]] == [N, P, Q] and val(a[7]) == 0
    assert val(a[6]) == 10.0 * np.sqrt(np.var(Y5, ddof=1))
    assert (ctx.p, ctx.q, ctx.n, ctx.d, ctx.device, ctx.handle) == (P, Q, N, D, 0, H)
    make_ctx(fake, max_stdev=3, device=1)
    a = fake.args("carma_ctx_create")
    assert val(a[6]) == 3.0 and isinstance(val(a[6]), float) and val(a[7]) == 1
    L.Context([1.0], [2.0], [0.1], 1)                          # one datum: no sample variance
    assert val(fake.args("carma_ctx_create")[6]) == 0.0 and val(fake.args("carma_ctx_create")[5]) == 0
    with pytest.raises(ValueError, match="time, y, yerr must have the same length"):
        L.Context(T5, Y5[:4], E5, P, Q)


def test_kalman_handle(fake):
    kf = _kf_car1(fake, device=2)
    a = fake.args("carma_kf_create_car1")
    assert rd(a[1], (N,)).tolist() == Y5.tolist() and [val(x) for x in a[3:]] == [N, 2.0, 0.25, 2]
    kf = _kf_carma(fake)
    a = fake.args("carma_kf_create_carma")
    assert [val(a[3]), val(a[4]), val(a[5]), val(a[8]), val(a[9])] == [N, P, 2.0, 2, 0]
    assert np.array_equal(rd(a[6], (P, 2)), REIM3[0]) and rd(a[7], (2,)).tolist() == [1.0, 0.5]
    assert kf.n == N
    fake.on["carma_kf_filter"] = lambda h, m, v: (fill(m, (N,)), fill(v, (N,), 10), 0)[2]
    mean, var = kf.filter()
    assert mean.tolist() == list(range(5)) and var.tolist() == list(range(10, 15))
    fake.on["carma_kf_predict"] = lambda h, tp, M, pm, pv: (fill(pm, (M,)), fill(pv, (M,), 10), 0)[2]
    pm, pv = kf.predict(7.5)                                   # a scalar is one time
    a = fake.args("carma_kf_predict")
    assert a[0] == H and rd(a[1], (1,)).tolist() == [7.5] and val(a[2]) == 1 and pm.tolist() == [0.0] and pv.tolist() == [10.0]
    for name, call in (("carma_kf_filter", kf.filter), ("carma_kf_predict", lambda: kf.predict([1.0, 2.0]))):
        fake.on[name] = lambda *a: 1
        with pytest.raises(L.CarmaError) as e:
            call()
        assert str(e.value) == "KalmanFilterp: singular eigenvector matrix (solve failed)"
        fake.on[name] = lambda *a: -5
        with pytest.raises(L.CarmaError, match=r"%s failed \(-5\)" % name):
            call()


def test_comm(fake):
    fake.on["carma_comm_unique_id"] = lambda buf: (C.memmove(buf, b"\x01\x02" * 64, 128), 0)[1]
    uid = L.Comm.unique_id()
    assert uid == b"\x01\x02" * 64
    comm = L.Comm(uid, 4, 1, device=3)
    a = fake.args("carma_comm_create")
    assert a[0].raw == uid and [val(x) for x in a[1:]] == [4, 1, 3] and (comm.rank, comm.size, comm.device) == (1, 4, 3)

    class Dist:
        def __init__(self, rank):
            self.rank, self.sent = rank, None

        def get_rank(self):
            return self.rank

        def get_world_size(self):
            return 2

        def broadcast_object_list(self, box, src):
            assert src == 0 and (box[0] is None) == (self.rank != 0)
            box[0] = uid

    for rank in (0, 1):
        n = fake.count("carma_comm_unique_id")
        c = L.Comm.from_torch(Dist(rank), device=0)
        assert fake.count("carma_comm_unique_id") == n + (rank == 0) and (c.rank, c.size) == (rank, 2)


# ---- Context ----------------------------------------------------------------------------------------
def test_context_calls(fake):
    ctx = make_ctx(fake)
    fake.on["carma_ctx_get_data"] = lambda h, t, y, e: (fill(t, (N,)), fill(y, (N,), 10), fill(e, (N,), 20), 0)[3]
    assert [a.tolist() for a in ctx.data()] == [list(range(0, 5)), list(range(10, 15)), list(range(20, 25))]
    fake.on["carma_ctx_get_prior"] = lambda h, o: (fill(o, (3,), 1), 0)[1]
    assert ctx.prior() == (1.0, 2.0, 3.0)
    ctx.set_prior(4)
    assert fake.args("carma_ctx_set_prior") == (H, 4.0)
    seen = {}

    def logdens(h, th, B, ip, out):
        seen.update(th=rd(th, (B, D)), B=B, ip=ip)
        fill(out, (B,), 100)
        return 0
    fake.on["carma_logdensity_batch"] = logdens
    th = np.arange(2.0 * D).reshape(2, D)
    out = ctx.logdensity(th)
    assert out.tolist() == [100.0, 101.0] and np.array_equal(seen["th"], th) and (seen["B"], seen["ip"]) == (2, 0)
    out = ctx.logdensity(th[1], ignore_prior=True)
    assert isinstance(out, float) and out == 100.0 and np.array_equal(seen["th"], th[1:]) and (seen["B"], seen["ip"]) == (1, 1)
    assert ctx.logdensity(np.zeros((3, 1, D))).shape == (3,)   # more axes: rows of d
    ctx.logdensity_dev(0x7000, 16, 0x8000, stream=0x9000)
    assert [val(x) for x in fake.args("carma_logdensity_batch_dev")] == [H, 0x7000, 16, 0, 0x8000, 0x9000]
    ctx.logdensity_dev(0x7000, 16, 0x8000, ignore_prior=True)
    assert [val(x) for x in fake.args("carma_logdensity_batch_dev")][3:] == [1, 0x8000, None]     # stream 0 is NULL
    fake.on["carma_logdensity_kernel_name"] = lambda h, B, buf, n: (setattr(buf, "value", b"k_%d_%d" % (B, n)), 0)[1]
    assert ctx.kernel_name(512) == "k_512_128"
    fake.on["carma_logprior"] = lambda h, th: float(rd(th, (D,)).sum())
    assert ctx.logprior(np.arange(6)) == 15.0


def _script_mle(fake, name, nlead, B, d, seen):
    def mle(*a):
        seen["a"] = a
        x, fun, nit, nfev, status = a[nlead + 6:]
        fill(x, (B, d)), fill(fun, (B,), 50), fill(nit, (B,), 1, np.int32), fill(nfev, (B,), 11, np.int32), fill(status, (B,), 21, np.int32)
        return 0
    fake.on[name] = mle


def _check_mle_out(res, B, d):
    x, fun, nit, nfev, status = res
    assert np.array_equal(x, np.arange(B * d).reshape(B, d)) and fun.tolist() == [50.0 + i for i in range(B)]
    assert [a.dtype for a in (nit, nfev, status)] == [np.int32] * 3
    assert (nit.tolist(), nfev.tolist(), status.tolist()) == ([1 + i for i in range(B)], [11 + i for i in range(B)], [21 + i for i in range(B)])


def test_context_mle_batched(fake):
    ctx = make_ctx(fake)
    seen = {}
    _script_mle(fake, "carma_mle_batched", 5, 3, D, seen)
    x0 = np.arange(3.0 * D).reshape(3, D)
    bounds = [(None, 1.0), (-2.0, None), (None, None), (0.0, 5.0), (None, 6), (-7, None)]
    _check_mle_out(ctx.mle_batched(x0, bounds, maxiter=17, mem=4, ftol=1e-3, gtol=1e-4, fd_step=1e-2, ignore_prior=False), 3, D)
    a = seen["a"]
    assert a[0] == H and np.array_equal(rd(a[1], (3, D)), x0) and val(a[2]) == 3
    assert rd(a[3], (D,)).tolist() == [-np.inf, -2.0, -np.inf, 0.0, -np.inf, -7.0]
    assert rd(a[4], (D,)).tolist() == [1.0, np.inf, np.inf, 5.0, 6.0, np.inf]
    assert [val(v) for v in a[5:11]] == [17, 4, 1e-3, 1e-4, 1e-2, 0]
    seen.clear()
    _script_mle(fake, "carma_mle_batched", 5, 1, D, seen)
    _check_mle_out(ctx.mle_batched(x0[0], bounds), 1, D)       # one start: [d] is [1, d]
    assert [val(v) for v in seen["a"][5:11]] == [2000, 8, 2.220446049250313e-09, 1e-5, 1e-6, 1]
    with pytest.raises(ValueError, match=r"x0 must be \[B, 6\]"):
        ctx.mle_batched(np.zeros((3, D + 1)), bounds)


def test_context_sampler(fake):
    ctx = make_ctx(fake)
    with pytest.raises(AttributeError):
        ctx.pt_get_chains()                                    # before pt_create a Context has no shape
    for seed, want in ((-1, 2 ** 64 - 1), (2 ** 64 + 5, 5), (0, 0)):
        ctx.pt_create(T, R, 40, seed=seed)
        a = fake.args("carma_pt_create")
        assert (a[0], val(a[1]), val(a[2]), val(a[4]), val(a[5])) == (H, T, R, 40, want) and null(a[3])
    ctx.pt_create(T, R, 40, temperatures=[1.0, 2.0, 4.0])
    assert rd(fake.args("carma_pt_create")[3], (T,)).tolist() == [1.0, 2.0, 4.0]
    for init in (None, []):
        ctx.pt_start(init)
        a = fake.args("carma_pt_start")
        assert a[0] == H and null(a[1]) and val(a[2]) == 0
    ctx.pt_start(np.arange(2.0 * D).reshape(2, D))
    a = fake.args("carma_pt_start")
    assert rd(a[1], (2 * D,)).tolist() == list(range(2 * D)) and val(a[2]) == 2 * D
    theta = np.arange(1.0 * R * T * D)
    ctx.pt_set_chains(theta)
    a = fake.args("carma_pt_set_chains")
    assert a[0] == H and rd(a[1], (R * T * D,)).tolist() == theta.tolist() and null(a[2])
    ctx.pt_set_chains(theta.reshape(R, T, D), logpost=np.arange(6.0))
    assert rd(fake.args("carma_pt_set_chains")[2], (R, T)).tolist() == [[0, 1, 2], [3, 4, 5]]
    with pytest.raises(ValueError):
        ctx.pt_set_chains(theta[:-1])
    fake.on["carma_pt_get_chains"] = lambda h, th, lp: (fill(th, (R, T, D)), fill(lp, (R, T), 100), 0)[2]
    th, lp = ctx.pt_get_chains()
    assert np.array_equal(th, theta.reshape(R, T, D)) and np.array_equal(lp, 100 + np.arange(6.0).reshape(R, T))
    fake.on["carma_pt_get_factor"] = lambda h, c: (fill(c, (R, T, D, D)), 0)[1]
    assert np.array_equal(ctx.pt_get_factor(), np.arange(1.0 * R * T * D * D).reshape(R, T, D, D))
    ctx.pt_set_factor(np.arange(1.0 * R * T * D * D))
    a = fake.args("carma_pt_set_factor")
    assert a[0] == H and rd(a[1], (R * T * D * D,)).tolist() == list(range(R * T * D * D))
    ctx.pt_iterate(9)
    ctx.pt_iterate(np.int64(8), do_exchange=False)
    assert [tuple(val(v) for v in a) for n, a in fake.calls if n == "carma_pt_iterate"] == [(H, 9, 1), (H, 8, 0)]
    fake.on["carma_pt_sample"] = lambda h, n, thin, s, lp: (fill(s, (R, n, D)), fill(lp, (R, n), 7), 0)[2]
    s, lp = ctx.pt_sample(4, thin=3)
    assert [val(v) for v in fake.args("carma_pt_sample")[:3]] == [H, 4, 3]
    assert np.array_equal(s, np.arange(1.0 * R * 4 * D).reshape(R, 4, D)) and np.array_equal(lp, 7 + np.arange(8.0).reshape(R, 4))
    fake.on["carma_pt_stats"] = lambda h, acc, swp, reset: (fill(acc, (R, T)), fill(swp, (R, T), 10), 0)[2]
    acc, swp = ctx.pt_stats(reset=True)
    assert val(fake.args("carma_pt_stats")[3]) == 1 and acc.tolist() == [[0, 1, 2], [3, 4, 5]] and swp.tolist() == [[10, 11, 12], [13, 14, 15]]
    ctx.pt_stats()
    assert val(fake.args("carma_pt_stats")[3]) == 0
    fake.on["carma_pt_iterations_done"] = lambda h: 77
    assert ctx.pt_iterations_done() == 77
    fake.on["carma_pt_iterate"] = lambda *a: -5
    with pytest.raises(L.CarmaError, match=r"carma_pt_iterate failed \(-5\)"):
        ctx.pt_iterate(1)


def test_context_pt_run_and_one_sided_members(fake):
    ctx = make_ctx(fake)
    S = 4
    fake.on["carma_pt_run"] = lambda *a: (fill(a[9], (R, S, D)), fill(a[10], (R, S), 5), 0)[2]
    for init, n in ((None, 0), ([], 0), (np.arange(1.0 * D), D)):
        s, lp = ctx.pt_run(T, R, S, 30, thin=2, init=init, seed=-1)
        a = fake.args("carma_pt_run")
        assert [val(v) for v in a[:6]] == [H, T, R, S, 30, 2] and null(a[6]) == (n == 0) and val(a[7]) == n and val(a[8]) == 2 ** 64 - 1
        assert np.array_equal(s, np.arange(1.0 * R * S * D).reshape(R, S, D)) and np.array_equal(lp, 5 + np.arange(8.0).reshape(R, S))
    assert ctx.pt_stats()[0].shape == (R, T)                  # pt_run left the shape
    ctx.pt_shard(8, 2, 1)
    assert [val(v) for v in fake.args("carma_pt_shard")] == [H, 8, 2, 1] and ctx._pt_slot0 == 2
    ctx.pt_bind_state(0x7000, 0x8000)
    assert [val(v) for v in fake.args("carma_pt_bind_state")] == [H, 0x7000, 0x8000]
    fake.on["carma_pt_debug_draws"] = lambda h, r, t, it, z, ua, us: (fill(z, (D,)), wr(ua, [0.25]), wr(us, [0.75]), 0)[3]
    z, ua, us = ctx.pt_debug_draws(1, 2, 2 ** 40)
    assert [val(v) for v in fake.args("carma_pt_debug_draws")[:4]] == [H, 1, 2, 2 ** 40]
    assert z.tolist() == list(range(D)) and (ua, us) == (0.25, 0.75) and isinstance(ua, float)
    for code, name in ((0, "ladder"), (1, "row"), (2, "lane"), (9, "ladder")):
        fake.on["carma_pt_kernel_in_use"] = lambda h, code=code: code
        assert ctx.pt_kernel() == name
    for code, name in ((0, "one-datum"), (1, "window"), (2, "two-sided"), (-1, None)):
        fake.on["carma_pt_row_pipeline"] = lambda code=code: code
        assert L.Context.pt_row_pipeline() == name
    fake.on["carma_pt_boundary_stats"] = lambda h, a, b: (setref(a, 2 ** 40), setref(b, 3), 0)[2]
    assert ctx.pt_boundary_stats() == (2 ** 40, 3)
    fake.on["carma_pt_boundary_check"] = lambda h: -1
    assert ctx.pt_boundary_check() == -1
    ctx.pt_sweep()
    assert fake.args("carma_pt_sweep") == (H,)


def test_sharded_calls(fake):
    c0, c1 = make_ctx(fake), make_ctx(fake)
    c1._h = H + 8
    for c in (c0, c1):
        c.pt_create(T, R, 10)
    comm = L.Comm(b"\0" * 128, 2, 0)
    comm._h = H + 16
    L.pt_iterate_sharded([c0, c1], 25, comm)
    a = fake.args("carma_pt_iterate_sharded")
    assert list(a[0]) == [H, H + 8] and [val(v) for v in a[1:]] == [2, 25, H + 16]
    L.pt_iterate_sharded([c0], 5)
    assert [val(v) for v in fake.args("carma_pt_iterate_sharded")[1:]] == [1, 5, None]
    fake.on["carma_pt_sample_sharded"] = lambda arr, k, n, thin, comm, s, lp: (
        None if null(s) else (fill(s, (R, n, D)), fill(lp, (R, n), 3)), 0)[1]
    s, lp = L.pt_sample_sharded([c0, c1], 4, thin=2, comm=comm)         # the owner of temperature 0
    a = fake.args("carma_pt_sample_sharded")
    assert list(a[0]) == [H, H + 8] and [val(v) for v in a[1:5]] == [2, 4, 2, H + 16]
    assert np.array_equal(s, np.arange(1.0 * R * 4 * D).reshape(R, 4, D)) and np.array_equal(lp, 3 + np.arange(8.0).reshape(R, 4))
    c0.pt_shard(2 * T, 1, 0)                                   # not the owner: _pt_slot0 != 0
    assert L.pt_sample_sharded([c0], 4) == (None, None)
    a = fake.args("carma_pt_sample_sharded")
    assert [val(v) for v in a[1:5]] == [1, 4, 1, None] and null(a[5]) and null(a[6])


# ---- MultiContext -------------------------------------------------------------------------------------
def test_multicontext_create(fake):
    mc = make_mctx(fake, device=1)
    a = fake.args("carma_mctx_create")
    assert [rd(a[i], (N,)).tolist() for i in range(3)] == [T5.tolist(), Y5.tolist(), E5.tolist()]
    assert rd(a[3], (3,), np.int64).tolist() == [0, 3, 5] and [val(v) for v in a[4:7]] == [2, P, Q] and val(a[8]) == 1
    assert rd(a[7], (2,)).tolist() == [10.0 * np.sqrt(np.var(Y5[:3], ddof=1)), 10.0 * np.sqrt(np.var(Y5[3:], ddof=1))]
    assert (mc.p, mc.q, mc.nseries, mc.d, mc.device, mc.handle) == (P, Q, 2, D, 1, H) and mc.n.tolist() == [3, 2] and mc.n.dtype == np.int64
    make_mctx(fake, max_stdev=7)
    assert rd(fake.args("carma_mctx_create")[7], (2,)).tolist() == [7.0, 7.0]
    make_mctx(fake, max_stdev=[1.0, 2.0])
    assert rd(fake.args("carma_mctx_create")[7], (2,)).tolist() == [1.0, 2.0]
    L.MultiContext([([3.0], [1.0], [0.1])], 1)                 # one datum: no sample variance
    assert rd(fake.args("carma_mctx_create")[7], (1,)).tolist() == [0.0]
    for series, msg in (([], "MultiContext needs at least one series"), ([SERIES[0], SERIES[1][:2]], r"series 1: expected \(t, y, yerr\)"),
                        ([(T5[:3], Y5[:2], E5[:3])], "series 0: time, y, yerr must have the same length")):
        with pytest.raises(ValueError, match=msg):
            L.MultiContext(series, P, Q)
    fake.on["carma_mctx_get_data"] = lambda h, s, t, y, e: (fill(t, (mc.n[s],)), fill(y, (mc.n[s],), 10), fill(e, (mc.n[s],), 20), 0)[3]
    assert [a.tolist() for a in mc.data(1)] == [[0, 1], [10, 11], [20, 21]] and val(fake.args("carma_mctx_get_data")[1]) == 1
    fake.on["carma_mctx_get_prior"] = lambda h, s, o: (fill(o, (3,), s), 0)[1]
    assert mc.prior(1) == (1.0, 2.0, 3.0)
    fake.on["carma_mlogdensity_kernel_name"] = lambda h, buf, n: (setattr(buf, "value", b"k_ms_%d" % n), 0)[1]
    assert mc.kernel_name() == "k_ms_128"


def test_multicontext_logdensity_and_which(fake):
    mc = make_mctx(fake)
    seen = {}

    def logdens(h, th, w, B, ip, out):
        seen.update(th=rd(th, (B, D)), w=rd(w, (B,), np.int32).tolist(), ip=ip)
        fill(out, (B,), 100)
        return 0
    fake.on["carma_mlogdensity_batch"] = logdens
    th = np.arange(3.0 * D).reshape(3, D)
    assert mc.logdensity(th, 1).tolist() == [100.0, 101.0, 102.0] and seen["w"] == [1, 1, 1] and np.array_equal(seen["th"], th)
    assert mc.logdensity(th, [1, 0, 1], ignore_prior=True).shape == (3,) and seen["w"] == [1, 0, 1] and seen["ip"] == 1
    out = mc.logdensity(th[2], 0)
    assert isinstance(out, float) and out == 100.0 and seen["w"] == [0]
    for which in (2, [0, -1, 1]):
        with pytest.raises(ValueError, match=r"series index out of range \[0, 2\)"):
            mc.logdensity(th, which)
    with pytest.raises(ValueError):
        mc.logdensity(th, [0, 1])                              # two indices for three rows


def test_multicontext_items_errors(fake):
    mc = make_mctx(fake)
    who = "MultiContext.kfilter"
    for args, msg in (((0, [], ROOTS3[:0], MA3[:0]), who + ": need at least one item"),
                      ((0, SIG3, ROOTS3[:2], MA3), who + r": roots must be \[3, 3\] \(one row of p roots per item\)"),
                      ((0, SIG3, ROOTS3[:, :2], MA3), who + r": roots must be \[3, 3\]"),
                      ((0, SIG3, ROOTS3, MA3[:2]), who + r": ma must be \[3, nma\] with 1 <= nma <= 3"),
                      ((0, SIG3, ROOTS3, np.ones((3, 4))), who + r": ma must be \[3, nma\] with 1 <= nma <= 3"),
                      ((0, SIG3, ROOTS3, np.ones((1, 3, 2))), who + r": ma must be \[3, nma\]"),
                      ((2, SIG3, ROOTS3, MA3), r"series index out of range \[0, 2\)")):
        with pytest.raises(ValueError, match=msg):
            mc.kfilter(*args)
    with pytest.raises(ValueError, match=who + ": mu must have one entry per item"):
        mc.kfilter(0, SIG3, ROOTS3, MA3, mu=[1.0, 2.0])
    with pytest.raises(ValueError, match="MultiContext.predict: need at least one item"):
        mc.predict(0, [], ROOTS3[:0], MA3[:0], [])
    with pytest.raises(ValueError, match="MultiContext.smooth: mu must have one entry per item"):
        mc.smooth(0, SIG3, ROOTS3, MA3, [[1.0]] * 3, mu=[1.0])
    m1 = make_mctx(fake, p=1)
    with pytest.raises(ValueError, match=who + r": roots must hold one root \(-omega\) per item for a CAR\(1\) context"):
        m1.kfilter(0, SIG3, [-0.5, -0.25], None)
    assert fake.count("carma_mkfilter") == 0


def test_multicontext_kfilter(fake):
    mc = make_mctx(fake)
    seen = {}

    def kf(h, w, M, sig, om, ma, nma, mu, mean, var, off, sing):
        seen.update(w=rd(w, (M,), np.int32).tolist(), M=M, sig=rd(sig, (M,)), om=rd(om, (M, P, 2)), ma=rd(ma, (M, nma)), nma=nma,
                    mu=None if null(mu) else rd(mu, (M,)).tolist(), off=off)
        fill(mean, (7,)), fill(var, (7,), 10), wr(sing, [0, 1, 0], np.int32)
        return 0
    fake.on["carma_mkfilter"] = kf
    means, vars_, sing = mc.kfilter([1, 0, 1], SIG3, ROOTS3, MA3)
    assert seen["w"] == [1, 0, 1] and seen["M"] == 3 and seen["nma"] == 2 and seen["mu"] is None and seen["off"] is None
    assert np.array_equal(seen["sig"], SIG3) and np.array_equal(seen["om"], REIM3) and np.array_equal(seen["ma"], MA3)
    assert [m.tolist() for m in means] == [[0, 1], [2, 3, 4], [5, 6]] and [v.tolist() for v in vars_] == [[10, 11], [12, 13, 14], [15, 16]]
    assert sing.dtype == bool and sing.tolist() == [False, True, False]
    mc.kfilter(0, SIG3, ROOTS3, MA3, mu=[1.0, 2.0, 3.0])
    assert seen["w"] == [0, 0, 0] and seen["mu"] == [1.0, 2.0, 3.0]
    m1 = make_mctx(fake, p=1)                                   # CAR(1): roots [M], ma ignored (ones)

    def kf1(h, w, M, sig, om, ma, nma, mu, mean, var, off, sing):
        seen.update(om=rd(om, (M, 2)), ma=rd(ma, (M, nma)).tolist(), nma=nma)
        return 0
    fake.on["carma_mkfilter"] = kf1
    m1.kfilter(0, SIG3, [-0.5, -0.25, -0.125], None)
    assert seen["om"].tolist() == [[-0.5, 0], [-0.25, 0], [-0.125, 0]] and seen["ma"] == [[1.0]] * 3 and seen["nma"] == 1


@pytest.mark.parametrize("method,cname", [("predict", "carma_mpredict"), ("smooth", "carma_msmooth")])
def test_multicontext_items_at_times(fake, method, cname):
    mc = make_mctx(fake)
    call = getattr(mc, method)
    seen = {}

    def script(flags, ntot):
        def at(h, w, M, sig, om, ma, nma, mu, tp, toff, pm, pv, sing):
            seen.update(w=rd(w, (M,), np.int32).tolist(), M=M, sig=rd(sig, (M,)), om=rd(om, (M, P, 2)), ma=rd(ma, (M, nma)), nma=nma,
                        mu=None if null(mu) else rd(mu, (M,)).tolist(), tp=rd(tp, (max(ntot, 1),)).tolist(),
                        toff=rd(toff, (M + 1,), np.int64).tolist())
            fill(pm, (max(ntot, 1),)), fill(pv, (max(ntot, 1),), 10), wr(sing, flags, np.int32)
            return 0
        fake.on[cname] = at
    script([0, 0, 0], 3)
    pm, pv = call([1, 0, 1], SIG3, ROOTS3, MA3, [[1.0, 2.0], [], 3.0], mu=[4.0, 5.0, 6.0])
    assert seen["w"] == [1, 0, 1] and seen["tp"] == [1.0, 2.0, 3.0] and seen["toff"] == [0, 2, 2, 3] and seen["mu"] == [4.0, 5.0, 6.0]
    assert np.array_equal(seen["sig"], SIG3) and np.array_equal(seen["om"], REIM3) and np.array_equal(seen["ma"], MA3) and seen["nma"] == 2
    assert [a.tolist() for a in pm] == [[0, 1], [], [2]] and [a.tolist() for a in pv] == [[10, 11], [], [12]]
    script([0, 0, 0], 0)                                        # every array empty: one dummy time, outputs of length 1
    res = call(0, SIG3, ROOTS3, MA3, [[], [], []])
    assert seen["tp"] == [0.0] and seen["toff"] == [0, 0, 0, 0] and seen["mu"] is None
    assert len(res) == 2 and [a.shape for a in res[0] + res[1]] == [(0,)] * 6
    with pytest.raises(ValueError) as e:
        call(0, SIG3, ROOTS3, MA3, [[1.0], [2.0]])
    assert str(e.value) == "MultiContext.%s: times must hold one array per item (3), got 2" % method
    script([0, 1, 1], 3)
    with pytest.raises(L.CarmaError) as e:
        call(0, SIG3, ROOTS3, MA3, [[1.0], [2.0], [3.0]])
    assert str(e.value) == "KalmanFilterp: singular eigenvector matrix (solve failed) for item(s) [1, 2]"
    pm, pv, sing = call(0, SIG3, ROOTS3, MA3, [[1.0], [2.0], [3.0]], return_singular=True)
    assert [a.tolist() for a in pm] == [[0], [1], [2]] and [a.tolist() for a in pv] == [[10], [11], [12]]
    assert sing.dtype == bool and sing.tolist() == [False, True, True]
    script([0, 0, 0], 3)
    assert len(call(0, SIG3, ROOTS3, MA3, [[1.0], [2.0], [3.0]], return_singular=True)) == 3
    M = 10                                                      # at most 8 indices in the message
    script([1] * M, M)
    with pytest.raises(L.CarmaError, match=r"for item\(s\) \[0, 1, 2, 3, 4, 5, 6, 7\]$"):
        call(0, np.ones(M), np.tile(ROOTS, (M, 1)), np.ones((M, 1)), [[1.0]] * M)
    fake.on[cname] = lambda *a: -22
    with pytest.raises(ValueError, match=r"%s failed \(-22\)" % cname):
        call(0, SIG3, ROOTS3, MA3, [[1.0], [2.0], [3.0]])


def test_multicontext_mle_batched(fake):
    mc = make_mctx(fake)
    seen = {}
    _script_mle(fake, "carma_mle_batched_ms", 6, 3, D, seen)
    x0 = np.arange(3.0 * D).reshape(3, D)
    lo, hi = -np.arange(1.0, D + 1), np.arange(3.0 * D).reshape(3, D) + 1
    _check_mle_out(mc.mle_batched(x0, [1, 0, 1], lo, hi, maxiter=9, ignore_prior=False), 3, D)
    a = seen["a"]
    assert a[0] == H and np.array_equal(rd(a[1], (3, D)), x0) and rd(a[2], (3,), np.int32).tolist() == [1, 0, 1] and val(a[3]) == 3
    assert np.array_equal(rd(a[4], (3, D)), np.tile(lo, (3, 1))) and np.array_equal(rd(a[5], (3, D)), hi)
    assert [val(v) for v in a[6:12]] == [9, 8, 2.220446049250313e-09, 1e-5, 1e-6, 0]
    with pytest.raises(ValueError, match=r"x0 must be \[B, 6\]"):
        mc.mle_batched(np.zeros((3, D - 1)), 0, lo, hi)
    with pytest.raises(ValueError, match="series index out of range"):
        mc.mle_batched(x0, 5, lo, hi)


def test_multicontext_sampler(fake):
    mc = make_mctx(fake)
    M = 3
    for call in (mc.pt_start, lambda: mc.pt_set_chains(np.zeros(M * R * T * D)), mc.pt_get_chains, mc.pt_get_factor,
                 lambda: mc.pt_set_factor(np.zeros(1)), lambda: mc.pt_sample(2), mc.pt_stats, lambda: mc.pt_logdensity(np.zeros(1))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "call pt_create first"
    with pytest.raises(ValueError, match="need at least one run"):
        mc.pt_create([], T, R, 10)
    with pytest.raises(ValueError, match="temperatures must hold ntemps = 3 values"):
        mc.pt_create([0], T, R, 10, temperatures=[1.0, 2.0])
    mc.pt_create([1, 0, 1], T, R, 40, seed=2 ** 64 + 5)
    a = fake.args("carma_mpt_create")
    assert a[0] == H and rd(a[1], (M,), np.int32).tolist() == [1, 0, 1] and [val(v) for v in a[2:5]] == [M, T, R] and null(a[5])
    assert [val(v) for v in a[6:]] == [40, 5]
    mc.pt_create([1, 0, 1], T, R, 40, seed=-1, temperatures=[1.0, 2.0, 4.0])
    a = fake.args("carma_mpt_create")
    assert rd(a[5], (T,)).tolist() == [1.0, 2.0, 4.0] and val(a[7]) == 2 ** 64 - 1
    mc.pt_start()
    assert fake.args("carma_mpt_start")[0] == H and null(fake.args("carma_mpt_start")[1])
    init = np.arange(1.0 * M * D).reshape(M, D)
    mc.pt_start(init)
    assert np.array_equal(rd(fake.args("carma_mpt_start")[1], (M, D)), init)
    with pytest.raises(ValueError, match=r"init must be \[3, 6\] \(one row per run\), got \(2, 6\)"):
        mc.pt_start(init[:2])
    lead = (M, R, T)
    theta = np.arange(1.0 * M * R * T * D)
    mc.pt_set_chains(theta)
    a = fake.args("carma_mpt_set_chains")
    assert a[0] == H and rd(a[1], theta.shape).tolist() == theta.tolist() and null(a[2])
    mc.pt_set_chains(theta.reshape(lead + (D,)), logpost=np.arange(18.0))
    assert rd(fake.args("carma_mpt_set_chains")[2], (18,)).tolist() == list(range(18))
    fake.on["carma_mpt_get_chains"] = lambda h, th, lp: (fill(th, lead + (D,)), fill(lp, lead, 100), 0)[2]
    th, lp = mc.pt_get_chains()
    assert np.array_equal(th, theta.reshape(lead + (D,))) and np.array_equal(lp, 100 + np.arange(18.0).reshape(lead))
    fake.on["carma_mpt_get_factor"] = lambda h, c: (fill(c, lead + (D, D)), 0)[1]
    assert np.array_equal(mc.pt_get_factor(), np.arange(18.0 * D * D).reshape(lead + (D, D)))
    mc.pt_set_factor(np.arange(18.0 * D * D))
    assert rd(fake.args("carma_mpt_set_factor")[1], (18 * D * D,)).tolist() == list(range(18 * D * D))
    mc.pt_iterate(9, do_exchange=False)
    assert [val(v) for v in fake.args("carma_mpt_iterate")] == [H, 9, 0]
    fake.on["carma_mpt_sample"] = lambda h, n, thin, s, lp: (fill(s, (M, R, n, D)), fill(lp, (M, R, n), 7), 0)[2]
    s, lp = mc.pt_sample(4, thin=3)
    assert [val(v) for v in fake.args("carma_mpt_sample")[:3]] == [H, 4, 3]
    assert np.array_equal(s, np.arange(1.0 * M * R * 4 * D).reshape(M, R, 4, D)) and np.array_equal(lp, 7 + np.arange(24.0).reshape(M, R, 4))
    fake.on["carma_mpt_stats"] = lambda h, acc, swp, reset: (fill(acc, lead), fill(swp, lead, 50), 0)[2]
    acc, swp = mc.pt_stats(reset=True)
    assert val(fake.args("carma_mpt_stats")[3]) == 1 and np.array_equal(acc, np.arange(18.0).reshape(lead)) and swp[2, 1, 2] == 67.0
    fake.on["carma_mpt_iterations_done"] = lambda h: 2 ** 33
    assert mc.pt_iterations_done() == 2 ** 33
    fake.on["carma_mpt_logdensity"] = lambda h, th, out: (fill(out, lead, rd(th, (1,))[0]), 0)[1]
    assert np.array_equal(mc.pt_logdensity(theta + 3), 3 + np.arange(18.0).reshape(lead))
    fake.on["carma_mpt_kernel_name"] = lambda h, buf, n: (setattr(buf, "value", b"k_mpt"), 0)[1]
    assert mc.pt_kernel_name() == "k_mpt"


def test_multicontext_pt_run_sets_the_shape(fake):
    mc = make_mctx(fake)
    M, S = 3, 4
    fake.on["carma_mpt_run"] = lambda *a: (fill(a[10], (a[2], R, S, D)), fill(a[11], (a[2], R, S), 5), 0)[2]
    init = np.arange(1.0 * M * D).reshape(M, D)
    s, lp = mc.pt_run([1, 0, 1], T, R, S, 30, thin=2, init=init, seed=-1)
    a = fake.args("carma_mpt_run")
    assert a[0] == H and rd(a[1], (M,), np.int32).tolist() == [1, 0, 1] and [val(v) for v in a[2:8]] == [M, T, R, S, 30, 2]
    assert np.array_equal(rd(a[8], (M, D)), init) and val(a[9]) == 2 ** 64 - 1
    assert np.array_equal(s, np.arange(1.0 * M * R * S * D).reshape(M, R, S, D)) and np.array_equal(lp, 5 + np.arange(24.0).reshape(M, R, S))
    assert mc.pt_stats()[0].shape == (M, R, T)
    mc.pt_run([0], T, R, S, 30)
    assert null(fake.args("carma_mpt_run")[8]) and mc.pt_stats()[0].shape == (1, R, T)
    with pytest.raises(ValueError, match=r"init must be \[1, 6\]"):
        mc.pt_run([0], T, R, S, 30, init=init)


# ---- BandsContext -------------------------------------------------------------------------------------
def test_bandscontext(fake):
    bc = make_bands(fake, K=2, device=1)
    a = fake.args("carma_bands_create")
    assert [rd(a[i], (N,)).tolist() for i in range(3)] == [T5.tolist(), Y5.tolist(), E5.tolist()]
    assert rd(a[3], (3,), np.int64).tolist() == [0, 3, 5] and [val(v) for v in a[4:7]] == [2, P, Q]
    assert rd(a[7], (1,)).tolist() == [-1.0] and rd(a[8], (1,)).tolist() == [1.5]
    assert val(a[9]) == 10.0 * np.sqrt(np.var(Y5[:3], ddof=1)) and val(a[10]) == 1      # band 0 sets the default max_stdev
    assert (bc.nbands, bc.dx, bc.d, bc.p, bc.q, bc.handle) == (2, D + 3, D, P, Q, H) and bc.n.tolist() == [3, 2]
    assert bc.lag_bounds.tolist() == [[-1.0, 1.5]]
    b1 = make_bands(fake, K=1, max_stdev=2)
    a = fake.args("carma_bands_create")
    assert null(a[7]) and null(a[8]) and val(a[4]) == 1 and val(a[9]) == 2.0 and (b1.dx, b1.d) == (D, D) and b1.lag_bounds.shape == (0, 2)
    for K, lb in ((2, None), (2, [(-1, 1), (-2, 2)]), (1, [(-1, 1)])):
        with pytest.raises(ValueError, match="lag_bounds must hold one \\(lo, hi\\) pair for each of the %d bands after the first" % (K - 1)):
            L.BandsContext(SERIES[:K], P, Q, lag_bounds=lb)
    for bands, msg in (([], "BandsContext needs at least one band"), ([SERIES[0], SERIES[1][:2]], r"band 1: expected \(t, y, yerr\)"),
                       ([(T5[:3], Y5[:2], E5[:3])], "band 0: time, y, yerr must have the same length")):
        with pytest.raises(ValueError, match=msg):
            L.BandsContext(bands, P, Q)
    fake.on["carma_bands_get_prior"] = lambda h, o: (fill(o, (3,), 1), 0)[1]
    assert bc.prior() == (1.0, 2.0, 3.0)
    seen = {}

    def logdens(h, th, B, ip, out):
        seen.update(th=rd(th, (B, bc.dx)), ip=ip)
        fill(out, (B,), 100)
        return 0
    fake.on["carma_bands_logdensity_batch"] = logdens
    th = np.arange(2.0 * bc.dx).reshape(2, bc.dx)
    assert bc.logdensity(th, ignore_prior=True).tolist() == [100.0, 101.0] and np.array_equal(seen["th"], th) and seen["ip"] == 1
    assert isinstance(bc.logdensity(th[0]), float)
    bc.logdensity_dev(0x7000, 16, 0x8000, stream=0x9000)
    assert [val(x) for x in fake.args("carma_bands_logdensity_batch_dev")] == [H, 0x7000, 16, 0, 0x8000, 0x9000]


def test_bandscontext_mle_batched(fake):
    bc = make_bands(fake, K=2)
    dx = bc.dx
    seen = {}
    _script_mle(fake, "carma_bands_mle_batched", 6, 3, dx, seen)
    x0 = np.arange(3.0 * dx).reshape(3, dx)
    _check_mle_out(bc.mle_batched(x0), 3, dx)
    a = seen["a"]
    assert a[0] == H and np.array_equal(rd(a[1], (3, dx)), x0) and val(a[2]) == 3 and null(a[5])
    assert rd(a[3], (dx,)).tolist() == [-np.inf] * dx and rd(a[4], (dx,)).tolist() == [np.inf] * dx
    assert [val(v) for v in a[6:12]] == [2000, 8, 2.220446049250313e-09, 1e-5, 1e-6, 1]
    _check_mle_out(bc.mle_batched(x0, lo=-np.arange(1.0 * dx), hi=np.arange(1.0 * dx), fixed_lag=[0.5, 1.5, 2.5], mem=3), 3, dx)
    a = seen["a"]
    assert rd(a[3], (dx,)).tolist() == (-np.arange(1.0 * dx)).tolist() and rd(a[4], (dx,)).tolist() == list(range(dx))
    assert rd(a[5], (3, 1)).tolist() == [[0.5], [1.5], [2.5]] and val(a[7]) == 3
    with pytest.raises(ValueError, match=r"x0 must be \[B, 9\]"):
        bc.mle_batched(np.zeros((3, D)))
    with pytest.raises(ValueError):
        bc.mle_batched(x0, fixed_lag=[0.5, 1.5])


def test_bandscontext_sampler_band_box_and_failed_calls(fake):
    bc = make_bands(fake, K=2)
    dx, S = bc.dx, 4
    for call in (lambda: bc.pt_set_chains(np.zeros(R * T * dx)), bc.pt_get_chains, bc.pt_stats, lambda: bc.pt_logdensity(np.zeros(1))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "call pt_create first"
    bc.pt_start()                                              # (one object has no run count to look up: the library's check)
    assert fake.count("carma_bands_pt_start") == 1
    with pytest.raises(ValueError, match="temperatures must hold ntemps = 3 values"):
        bc.pt_create(T, R, 10, temperatures=[1.0, 2.0])
    bc.pt_create(T, R, 40, seed=-1, temperatures=[1.0, 2.0, 4.0])
    a = fake.args("carma_bands_pt_create")
    assert a[0] == H and [val(v) for v in a[1:3]] == [T, R] and rd(a[3], (T,)).tolist() == [1.0, 2.0, 4.0]
    assert [val(v) for v in a[4:6]] == [40, 2 ** 64 - 1] and null(a[6]) and null(a[7]) and bc._pt_shape == (R, T)
    box = (np.array([[-1.0, -2.0]]), [3.0, 4.0])               # [K - 1, 2], or anything of its size
    bc.pt_create(T, R, 40, band_box=box)
    a = fake.args("carma_bands_pt_create")
    assert null(a[3]) and rd(a[6], (1, 2)).tolist() == [[-1.0, -2.0]] and rd(a[7], (1, 2)).tolist() == [[3.0, 4.0]]
    with pytest.raises(ValueError):
        bc.pt_create(T, R, 40, band_box=(np.zeros((2, 2)), np.zeros((2, 2))))
    bc.pt_start()
    assert fake.args("carma_bands_pt_start")[0] == H and null(fake.args("carma_bands_pt_start")[1])
    init = np.arange(1.0 * dx)
    bc.pt_start(init)
    assert rd(fake.args("carma_bands_pt_start")[1], (dx,)).tolist() == init.tolist()
    with pytest.raises(ValueError, match=r"init must be \[9\], got \(1, 9\)"):
        bc.pt_start(init[None])
    fake.on["carma_bands_pt_run"] = lambda *a: (fill(a[10], (R, S, dx)), fill(a[11], (R, S), 5), 0)[2]
    s, lp = bc.pt_run(T, R, S, 30, thin=2, init=init, seed=7, band_box=box)
    a = fake.args("carma_bands_pt_run")
    assert a[0] == H and [val(v) for v in a[1:6]] == [T, R, S, 30, 2] and rd(a[6], (dx,)).tolist() == init.tolist() and val(a[7]) == 7
    assert rd(a[8], (1, 2)).tolist() == [[-1.0, -2.0]] and rd(a[9], (1, 2)).tolist() == [[3.0, 4.0]]
    assert np.array_equal(s, np.arange(1.0 * R * S * dx).reshape(R, S, dx)) and np.array_equal(lp, 5 + np.arange(8.0).reshape(R, S))
    bc.pt_run(T, R, S, 30)
    a = fake.args("carma_bands_pt_run")
    assert null(a[6]) and null(a[8]) and null(a[9]) and bc.pt_stats()[0].shape == (R, T)
    # a failed create or run leaves no sampler behind
    for name, call in (("carma_bands_pt_create", lambda: bc.pt_create(T, R, 40)), ("carma_bands_pt_run", lambda: bc.pt_run(T, R, S, 30))):
        bc.pt_create(T, R, 40)
        assert bc._pt_shape == (R, T)
        fake.on[name] = lambda *a: -22
        with pytest.raises(ValueError, match=r"%s failed \(-22\)" % name):
            call()
        assert bc._pt_shape is None
        with pytest.raises(ValueError) as e:
            bc.pt_get_chains()
        assert str(e.value) == "call pt_create first"
        del fake.on[name]


def test_multicontext_sampler_failed_calls(fake):
    mc = make_mctx(fake)
    for name, call in (("carma_mpt_create", lambda: mc.pt_create([0], T, R, 40)), ("carma_mpt_run", lambda: mc.pt_run([0], T, R, 4, 30))):
        mc.pt_create([1, 0, 1], T, R, 40)
        assert mc._pt_shape == (3, R, T)
        fake.on[name] = lambda *a: -22
        with pytest.raises(ValueError, match=r"%s failed \(-22\)" % name):
            call()
        assert mc._pt_shape is None                            # a failed create or run leaves no sampler behind
        del fake.on[name]


# ---- BandsSetContext ----------------------------------------------------------------------------------
OBJECTS = [SERIES, [(T5[:3] + 10.0, 2.0 * Y5[:3], E5[:3]), (T5[3:] + 10.0, 3.0 * Y5[3:], E5[3:])]]
DX = D + 3


def make_bandset(fake, K=2, **kw):
    fake.on.update(carma_bandset_nobjects=lambda h: 2, carma_bandset_nbands=lambda h: K, carma_bandset_dim=lambda h: D + 3 * (K - 1),
                   carma_bandset_n=lambda h, s, b: (3, 2)[b])
    if K == 2:
        kw.setdefault("lag_bounds", [(-1.0, 1.5)])
    return L.BandsSetContext([o[:K] for o in OBJECTS], P, Q, **kw)


def test_bandsetcontext_create(fake):
    bs = make_bandset(fake, device=1)
    a = fake.args("carma_bandset_create")
    cat = [np.concatenate([b[i] for o in OBJECTS for b in o]) for i in range(3)]
    assert [rd(a[i], (2 * N,)).tolist() for i in range(3)] == [c.tolist() for c in cat]
    assert rd(a[3], (5,), np.int64).tolist() == [0, 3, 5, 8, 10] and [val(v) for v in a[4:8]] == [2, 2, P, Q]
    assert rd(a[8], (2, 1)).tolist() == [[-1.0], [-1.0]] and rd(a[9], (2, 1)).tolist() == [[1.5], [1.5]]       # one box for all objects
    # band 0 of each object sets its default max_stdev
    assert rd(a[10], (2,)).tolist() == [10.0 * np.sqrt(np.var(Y5[:3], ddof=1)), 10.0 * np.sqrt(np.var(2.0 * Y5[:3], ddof=1))]
    assert val(a[11]) == 1 and len(a) == 12
    assert (bs.nobjects, bs.nbands, bs.dx, bs.d, bs.p, bs.q, bs.handle, bs.device) == (2, 2, DX, D, P, Q, H, 1)
    assert bs.n.tolist() == [[3, 2], [3, 2]] and bs.n.dtype == np.int64 and bs.lag_bounds.tolist() == [[[-1.0, 1.5]], [[-1.0, 1.5]]]
    assert [fake.args("carma_bandset_n", k)[1:] for k in range(4)] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    bs = make_bandset(fake, lag_bounds=[[(-1.0, 1.5)], [(-2.0, 2.5)]], max_stdev=2)                              # a box per object
    a = fake.args("carma_bandset_create")
    assert rd(a[8], (2, 1)).tolist() == [[-1.0], [-2.0]] and rd(a[9], (2, 1)).tolist() == [[1.5], [2.5]]
    assert rd(a[10], (2,)).tolist() == [2.0, 2.0] and val(a[11]) == 0 and bs.lag_bounds.tolist() == [[[-1.0, 1.5]], [[-2.0, 2.5]]]
    make_bandset(fake, max_stdev=[1, 2])
    assert rd(fake.args("carma_bandset_create")[10], (2,)).tolist() == [1.0, 2.0]
    b1 = make_bandset(fake, K=1)
    a = fake.args("carma_bandset_create")
    assert null(a[8]) and null(a[9]) and val(a[5]) == 1 and rd(a[3], (3,), np.int64).tolist() == [0, 3, 6]
    assert (b1.dx, b1.d) == (D, D) and b1.lag_bounds.shape == (2, 0, 2)
    for lb in (None, [(-1, 1), (-2, 2), (-3, 3)]):
        with pytest.raises(ValueError, match=r"lag_bounds must hold one \(lo, hi\) pair for each of the 1 bands after the first, for all "
                                             "objects or for each of the 2 objects"):
            L.BandsSetContext(OBJECTS, P, Q, lag_bounds=lb)
    for objects, msg in (([], "BandsSetContext needs at least one object"),
                         ([OBJECTS[0], OBJECTS[1][:1]], "object 1 has 1 bands, object 0 has 2: the objects of a set share their bands"),
                         ([OBJECTS[0], [OBJECTS[1][0], OBJECTS[1][1][:2]]], r"band 3: expected \(t, y, yerr\)"),
                         ([[(T5[:3], Y5[:2], E5[:3])]], "band 0: time, y, yerr must have the same length")):
        with pytest.raises(ValueError, match=msg):
            L.BandsSetContext(objects, P, Q, lag_bounds=[(-1.0, 1.5)])
    with pytest.raises(ValueError, match="operands could not be broadcast|broadcast"):
        make_bandset(fake, max_stdev=[1, 2, 3])


def test_bandsetcontext_prior_logdensity(fake):
    bs = make_bandset(fake)
    fake.on["carma_bandset_get_prior"] = lambda h, s, o: (fill(o, (3,), 1 + 10 * s), 0)[1]
    assert bs.prior(1) == (11.0, 12.0, 13.0) and [val(v) for v in fake.args("carma_bandset_get_prior")[:2]] == [H, 1]
    seen = {}

    def logdens(h, th, w, B, ip, out):
        seen.update(th=rd(th, (B, DX)), w=rd(w, (B,), np.int32).tolist(), B=B, ip=ip, out=C.cast(out, C.c_void_p).value)
        fill(out, (B,), 100)
        return 0
    fake.on["carma_bandset_logdensity_batch"] = logdens
    th = np.arange(3.0 * DX).reshape(3, DX)
    out = bs.logdensity(th, [1, 0, 1])
    assert out.tolist() == [100.0, 101.0, 102.0] and np.array_equal(seen["th"], th) and (seen["w"], seen["B"], seen["ip"]) == ([1, 0, 1], 3, 0)
    assert bs.logdensity(th, 1, ignore_prior=True).shape == (3,) and (seen["w"], seen["ip"]) == ([1, 1, 1], 1)
    one = bs.logdensity(th[2], 0)
    assert isinstance(one, float) and one == 100.0 and np.array_equal(seen["th"], th[2:]) and seen["w"] == [0]
    assert bs.logdensity(th, 7).shape == (3,) and seen["w"] == [7, 7, 7]          # the range is the library's check
    buf = np.full((2, 2), -1.0)
    out = bs.logdensity(th, [0, 1, 0], out=buf)                                  # the first B entries of a caller's array
    assert seen["out"] == buf.ctypes.data and buf.ravel().tolist() == [100.0, 101.0, 102.0, -1.0] and out.tolist() == [100.0, 101.0, 102.0]
    assert out.base is not None and np.shares_memory(out, buf)
    for bad in (np.zeros(2), np.zeros(3, dtype=np.float32), np.zeros((3, 2))[:, 0]):
        with pytest.raises(ValueError, match="out must be a contiguous float64 array of at least 3 entries"):
            bs.logdensity(th, 0, out=bad)
    with pytest.raises(ValueError):
        bs.logdensity(th, [0, 1])
    fake.on["carma_bandset_kernel_name"] = lambda h, buf, n: (setattr(buf, "value", b"k_set_%d" % n), 0)[1]
    assert bs.kernel_name() == "k_set_128"


def test_bandsetcontext_mle_batched(fake):
    bs = make_bandset(fake)
    seen = {}
    _script_mle(fake, "carma_bandset_mle_batched", 7, 3, DX, seen)
    x0 = np.arange(3.0 * DX).reshape(3, DX)
    _check_mle_out(bs.mle_batched(x0, [1, 0, 1]), 3, DX)
    a = seen["a"]
    assert a[0] == H and np.array_equal(rd(a[1], (3, DX)), x0) and rd(a[2], (3,), np.int32).tolist() == [1, 0, 1] and val(a[3]) == 3
    assert np.all(rd(a[4], (3, DX)) == -np.inf) and np.all(rd(a[5], (3, DX)) == np.inf) and null(a[6])
    assert [val(v) for v in a[7:13]] == [2000, 8, 2.220446049250313e-09, 1e-5, 1e-6, 1] and len(a) == 18
    lo, hi = -np.arange(1.0, DX + 1), np.arange(3.0 * DX).reshape(3, DX) + 1    # [dx] for every start, [B, dx] a box per start
    _check_mle_out(bs.mle_batched(x0, 0, lo, hi, fixed_lag=[0.5, 1.5, 2.5], maxiter=9, mem=3, ignore_prior=False), 3, DX)
    a = seen["a"]
    assert rd(a[2], (3,), np.int32).tolist() == [0, 0, 0]
    assert np.array_equal(rd(a[4], (3, DX)), np.tile(lo, (3, 1))) and np.array_equal(rd(a[5], (3, DX)), hi)
    assert rd(a[6], (3, 1)).tolist() == [[0.5], [1.5], [2.5]] and [val(v) for v in a[7:13]] == [9, 3, 2.220446049250313e-09, 1e-5, 1e-6, 0]
    with pytest.raises(ValueError, match=r"x0 must be \[B, 9\]"):
        bs.mle_batched(np.zeros((3, D)), 0)
    with pytest.raises(ValueError):
        bs.mle_batched(x0, 0, fixed_lag=[0.5, 1.5])


def test_bandsetcontext_smooth(fake):
    bs = make_bandset(fake)
    seen, flags = {}, [0, 0, 0]

    def smooth(h, th, w, bo, B, tp, toff, mean, var, inv):
        off = rd(toff, (B + 1,), np.int64)
        ntot = max(int(off[-1]), 1)
        seen.update(th=rd(th, (B, DX)), w=rd(w, (B,), np.int32).tolist(), bo=rd(bo, (B,), np.int32).tolist(), B=B, off=off.tolist(),
                    tp=rd(tp, (ntot,)).tolist())
        fill(mean, (ntot,)), fill(var, (ntot,), 10), wr(inv, flags, np.int32)
        return 0
    fake.on["carma_bandset_smooth"] = smooth
    th = np.arange(3.0 * DX).reshape(3, DX)
    m, v = bs.smooth(th, [1, 0, 1], 1, [9.0, 8.0])                               # one time array and one band for all rows
    assert fake.args("carma_bandset_smooth")[0] == H and np.array_equal(seen["th"], th)
    assert (seen["w"], seen["bo"], seen["B"], seen["off"], seen["tp"]) == ([1, 0, 1], [1, 1, 1], 3, [0, 2, 4, 6], [9.0, 8.0] * 3)
    assert [a.tolist() for a in m] == [[0.0, 1.0], [2.0, 3.0], [4.0, 5.0]] and [a.tolist() for a in v] == [[10.0, 11.0], [12.0, 13.0], [14.0, 15.0]]
    m, v = bs.smooth(th, 0, [0, 1, 0], np.array([9.0, 8.0]))
    assert (seen["w"], seen["bo"], seen["off"]) == ([0, 0, 0], [0, 1, 0], [0, 2, 4, 6])
    m, v = bs.smooth(th, 0, 0, [[9.0, 8.0, 7.0], [], [6.0]])                     # an array per row; an empty one is allowed
    assert (seen["off"], seen["tp"]) == ([0, 3, 3, 4], [9.0, 8.0, 7.0, 6.0]) and [a.tolist() for a in m] == [[0.0, 1.0, 2.0], [], [3.0]]
    assert [a.tolist() for a in v] == [[10.0, 11.0, 12.0], [], [13.0]]
    m, v = bs.smooth(th, 0, 0, np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]))   # [B, M]: a row of times per row
    assert (seen["off"], seen["tp"]) == ([0, 2, 4, 6], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    m, v = bs.smooth(th[0], 1, 0, 4.5)                                           # one vector is one row; one time is one time
    assert (seen["B"], seen["off"], seen["tp"]) == (1, [0, 1], [4.5]) and [a.tolist() for a in m] == [[0.0]]
    m, v = bs.smooth(th, 0, 0, [[], [], []])                                     # all empty: one dummy time, outputs of length 1
    assert (seen["off"], seen["tp"]) == ([0, 0, 0, 0], [0.0]) and [a.size for a in m] == [0, 0, 0]
    with pytest.raises(ValueError, match=r"BandsSetContext.smooth: times must hold one array per row \(3\), got 2"):
        bs.smooth(th, 0, 0, [[9.0], [8.0]])
    flags[:] = [0, 1, 1]
    m, v, inv = bs.smooth(th, 0, 0, [9.0, 8.0], return_invalid=True)
    assert inv.dtype == bool and inv.tolist() == [False, True, True] and len(m) == len(v) == 3
    with pytest.raises(L.CarmaError) as e:
        bs.smooth(th, 0, 0, [9.0, 8.0])
    assert str(e.value) == "BandsSetContext.smooth: a repeated AR root or a non-finite lag, scale or offset for row(s) [1, 2]"
    fake.on["carma_bandset_smooth"] = lambda *a: -22
    with pytest.raises(ValueError, match=r"carma_bandset_smooth failed \(-22\)"):
        bs.smooth(th, 0, 0, [9.0])


def test_bandsetcontext_sampler(fake):
    bs = make_bandset(fake)
    M, S = 3, 4
    fake.on["carma_bandset_pt_default_box"] = lambda h, s, lo, hi: (fill(lo, (1, 2), 10 * s), fill(hi, (1, 2), 10 * s + 5), 0)[2]
    lo, hi = bs.pt_default_box(1)
    assert [val(v) for v in fake.args("carma_bandset_pt_default_box")[:2]] == [H, 1] and lo.tolist() == [[10.0, 11.0]] and hi.tolist() == [[15.0, 16.0]]
    for call in (bs.pt_start, lambda: bs.pt_set_chains(np.zeros(M * R * T * DX)), bs.pt_get_chains, bs.pt_get_factor,
                 lambda: bs.pt_sample(2), bs.pt_stats, lambda: bs.pt_logdensity(np.zeros(1))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "call pt_create first"
    with pytest.raises(ValueError, match="need at least one run"):
        bs.pt_create([], T, R, 10)
    with pytest.raises(ValueError, match="temperatures must hold ntemps = 3 values"):
        bs.pt_create([0], T, R, 10, temperatures=[1.0, 2.0])
    bs.pt_create([1, 0, 1], T, R, 40, seed=2 ** 64 + 5)                          # band_box None: no box
    a = fake.args("carma_bandset_pt_create")
    assert a[0] == H and rd(a[1], (M,), np.int32).tolist() == [1, 0, 1] and [val(v) for v in a[2:5]] == [M, T, R] and null(a[5])
    assert [val(v) for v in a[6:8]] == [40, 5] and null(a[8]) and null(a[9]) and len(a) == 10 and bs._pt_shape == (M, R, T)
    one = (np.array([[-1.0, -2.0]]), np.array([[3.0, 4.0]]))                     # [K - 1, 2]: for every run
    bs.pt_create([1, 0, 1], T, R, 40, seed=-1, temperatures=[1.0, 2.0, 4.0], band_box=one)
    a = fake.args("carma_bandset_pt_create")
    assert rd(a[5], (T,)).tolist() == [1.0, 2.0, 4.0] and val(a[7]) == 2 ** 64 - 1
    assert rd(a[8], (M, 1, 2)).tolist() == [[[-1.0, -2.0]]] * M and rd(a[9], (M, 1, 2)).tolist() == [[[3.0, 4.0]]] * M
    per = (-np.arange(1.0, 2 * M + 1).reshape(M, 1, 2), np.arange(1.0, 2 * M + 1).reshape(M, 1, 2))      # [M, K - 1, 2]: a box per run
    bs.pt_create([1, 0, 1], T, R, 40, band_box=per)
    a = fake.args("carma_bandset_pt_create")
    assert np.array_equal(rd(a[8], (M, 1, 2)), per[0]) and np.array_equal(rd(a[9], (M, 1, 2)), per[1])
    with pytest.raises(ValueError):
        bs.pt_create([1, 0], T, R, 40, band_box=per)
    bs.pt_create([1, 0, 1], T, R, 40)
    bs.pt_start()
    assert fake.args("carma_bandset_pt_start")[0] == H and null(fake.args("carma_bandset_pt_start")[1])
    init = np.arange(1.0 * M * DX).reshape(M, DX)
    bs.pt_start(init)
    assert np.array_equal(rd(fake.args("carma_bandset_pt_start")[1], (M, DX)), init)
    with pytest.raises(ValueError, match=r"init must be \[3, 9\] \(one row per run\), got \(2, 9\)"):
        bs.pt_start(init[:2])
    lead = (M, R, T)
    fake.on["carma_bandset_pt_get_chains"] = lambda h, th, lp: (fill(th, lead + (DX,)), fill(lp, lead, 100), 0)[2]
    th, lp = bs.pt_get_chains()
    assert np.array_equal(th, np.arange(18.0 * DX).reshape(lead + (DX,))) and np.array_equal(lp, 100 + np.arange(18.0).reshape(lead))
    fake.on["carma_bandset_pt_sample"] = lambda h, n, thin, s, lp: (fill(s, (M, R, n, DX)), fill(lp, (M, R, n), 7), 0)[2]
    s, lp = bs.pt_sample(4, thin=3)
    assert np.array_equal(s, np.arange(1.0 * M * R * 4 * DX).reshape(M, R, 4, DX)) and lp.shape == (M, R, 4)
    fake.on["carma_bandset_pt_kernel_name"] = lambda h, buf, n: (setattr(buf, "value", b"k_bspt"), 0)[1]
    assert bs.pt_kernel_name() == "k_bspt"
    fake.on["carma_bandset_pt_run"] = lambda *a: (fill(a[12], (a[2], R, S, DX)), fill(a[13], (a[2], R, S), 5), 0)[2]
    s, lp = bs.pt_run([1, 0, 1], T, R, S, 30, thin=2, init=init, seed=-1, band_box=per)
    a = fake.args("carma_bandset_pt_run")
    assert a[0] == H and rd(a[1], (M,), np.int32).tolist() == [1, 0, 1] and [val(v) for v in a[2:8]] == [M, T, R, S, 30, 2]
    assert np.array_equal(rd(a[8], (M, DX)), init) and val(a[9]) == 2 ** 64 - 1 and len(a) == 14
    assert np.array_equal(rd(a[10], (M, 1, 2)), per[0]) and np.array_equal(rd(a[11], (M, 1, 2)), per[1])
    assert np.array_equal(s, np.arange(1.0 * M * R * S * DX).reshape(M, R, S, DX)) and np.array_equal(lp, 5 + np.arange(24.0).reshape(M, R, S))
    bs.pt_run([0, 1], T, R, S, 30, band_box=one)
    a = fake.args("carma_bandset_pt_run")
    assert null(a[8]) and rd(a[10], (2, 1, 2)).tolist() == [[[-1.0, -2.0]]] * 2 and rd(a[11], (2, 1, 2)).tolist() == [[[3.0, 4.0]]] * 2
    assert bs.pt_stats()[0].shape == (2, R, T)
    bs.pt_run([0], T, R, S, 30)
    a = fake.args("carma_bandset_pt_run")
    assert null(a[8]) and null(a[10]) and null(a[11]) and bs.pt_stats()[0].shape == (1, R, T)
    with pytest.raises(ValueError, match=r"init must be \[1, 9\]"):
        bs.pt_run([0], T, R, S, 30, init=init)
    # a failed create or run leaves no sampler behind
    for name, call in (("carma_bandset_pt_create", lambda: bs.pt_create([0], T, R, 40)),
                       ("carma_bandset_pt_run", lambda: bs.pt_run([0], T, R, S, 30))):
        bs.pt_create([1, 0, 1], T, R, 40)
        assert bs._pt_shape == (M, R, T)
        fake.on[name] = lambda *a: -22
        with pytest.raises(ValueError, match=r"%s failed \(-22\)" % name):
            call()
        assert bs._pt_shape is None
        with pytest.raises(ValueError) as e:
            bs.pt_stats()
        assert str(e.value) == "call pt_create first"
        del fake.on[name]


# ---- stateless calls -----------------------------------------------------------------------------------
def test_kfilter_single_truncates_to_nout(fake):
    def kf(*a):
        fill(a[9], (N,)), fill(a[10], (N,), 10), setref(a[11], 3)
        return 0
    fake.on["carma_kfilter_carma"] = kf
    mean, var = L.kfilter_carma(T5, Y5, E5, 2.0, ROOTS, MA3[0], device=1)
    a = fake.args("carma_kfilter_carma")
    assert [rd(a[i], (N,)).tolist() for i in range(3)] == [T5.tolist(), Y5.tolist(), E5.tolist()]
    assert [val(a[3]), val(a[4]), val(a[5]), val(a[8]), val(a[12])] == [N, P, 2.0, 2, 1]
    assert np.array_equal(rd(a[6], (P, 2)), REIM3[0]) and rd(a[7], (2,)).tolist() == [1.0, 0.5]
    assert mean.tolist() == [0, 1, 2] and var.tolist() == [10, 11, 12]
    fake.on["carma_kfilter_carma"] = lambda *a: 1
    with pytest.raises(L.CarmaError) as e:
        L.kfilter_carma(T5, Y5, E5, 2.0, ROOTS, MA3[0])
    assert str(e.value) == "KalmanFilterp: singular eigenvector matrix (solve failed)"
    fake.on["carma_kfilter_car1"] = lambda *a: (fill(a[6], (N,)), fill(a[7], (N,), 10), setref(a[8], 4), 0)[3]
    mean, var = L.kfilter_car1(T5, Y5, E5, 2, 0.25)
    a = fake.args("carma_kfilter_car1")
    assert [val(v) for v in a[3:6]] == [N, 2.0, 0.25] and val(a[9]) == 0 and mean.tolist() == [0, 1, 2, 3] and var.tolist() == [10, 11, 12, 13]
    fake.on["carma_kfilter_car1"] = lambda *a: -19
    with pytest.raises(L.CarmaDeviceError, match=r"carma_kfilter_car1 failed \(-19\)"):
        L.kfilter_car1(T5, Y5, E5, 2, 0.25)


def test_kfilter_carma_batch_rows_are_back_to_back(fake):
    B, m = 3, 4
    seen = {}

    def kf(*a):
        seen["a"] = a
        fill(a[11], (a[5] * N,)), fill(a[12], (a[5] * N,), 100), wr(a[13], [0, 0, 1][-a[5]:], np.int32), setref(a[14], m)
        return 0
    fake.on["carma_kfilter_batch_carma"] = kf
    mean, var, sing = L.kfilter_carma_batch(T5, Y5, E5, SIG3, ROOTS3, MA3, mu=[1.0, 2.0, 3.0], device=2)
    a = seen["a"]
    assert [val(v) for v in a[3:6]] == [N, P, B] and val(a[9]) == 2 and val(a[15]) == 2
    assert np.array_equal(rd(a[6], (B,)), SIG3) and np.array_equal(rd(a[7], (B, P, 2)), REIM3) and np.array_equal(rd(a[8], (B, 2)), MA3)
    assert rd(a[10], (B,)).tolist() == [1.0, 2.0, 3.0]
    assert np.array_equal(mean, np.arange(12.0).reshape(B, m)) and np.array_equal(var, 100 + np.arange(12.0).reshape(B, m))
    assert sing.dtype == bool and sing.tolist() == [False, False, True]
    L.kfilter_carma_batch(T5, Y5, E5, 2.0, ROOTS, MA3[0])       # one model: scalars and rows are promoted
    a = seen["a"]
    assert [val(v) for v in a[3:6]] == [N, P, 1] and null(a[10]) and val(a[15]) == 0
    for args in ((SIG3[:2], ROOTS3, MA3), (SIG3, ROOTS3, MA3[:2])):
        with pytest.raises(ValueError) as e:
            L.kfilter_carma_batch(T5, Y5, E5, *args)
        assert str(e.value) == "kfilter_carma_batch: sigsqr, omega and ma must describe the same number of models"
    with pytest.raises(ValueError) as e:
        L.kfilter_carma_batch(T5, Y5, E5, SIG3, ROOTS3, MA3, mu=[1.0])
    assert str(e.value) == "kfilter_carma_batch: mu must have one entry per model"


def test_predict_and_simulate(fake):
    fake.on["carma_predict_carma"] = lambda *a: (fill(a[11], (2,)), fill(a[12], (2,), 10), 0)[2]
    pm, pv = L.predict_carma(T5, Y5, E5, 2.0, ROOTS, MA3[0], [7.0, 6.0], device=1)
    a = fake.args("carma_predict_carma")
    assert [val(a[i]) for i in (3, 4, 5, 8, 10, 13)] == [N, P, 2.0, 2, 2, 1] and rd(a[9], (2,)).tolist() == [7.0, 6.0]      # not sorted
    assert np.array_equal(rd(a[6], (P, 2)), REIM3[0]) and pm.tolist() == [0, 1] and pv.tolist() == [10, 11]
    fake.on["carma_predict_carma"] = lambda *a: 1
    with pytest.raises(L.CarmaError) as e:
        L.predict_carma(T5, Y5, E5, 2.0, ROOTS, MA3[0], 7.0)
    assert str(e.value) == "KalmanFilterp: singular eigenvector matrix (solve failed)"
    fake.on["carma_predict_car1"] = lambda *a: (fill(a[8], (1,)), fill(a[9], (1,), 10), 0)[2]
    pm, pv = L.predict_car1(T5, Y5, E5, 2.0, 0.25, 7.0)
    a = fake.args("carma_predict_car1")
    assert [val(a[i]) for i in (3, 4, 5, 7, 10)] == [N, 2.0, 0.25, 1, 0] and rd(a[6], (1,)).tolist() == [7.0] and (pm[0], pv[0]) == (0, 10)
    fake.on["carma_simulate_carma"] = lambda *a: (fill(a[9], (2, 3)), 0)[1]
    out = L.simulate_carma([3.0, 1.0, 2.0], 2.0, ROOTS, MA3[0], npaths=2, seed=-1, device=1)
    a = fake.args("carma_simulate_carma")
    assert rd(a[0], (3,)).tolist() == [1.0, 2.0, 3.0] and [val(a[i]) for i in (1, 2, 3, 6, 7, 8, 10)] == [3, P, 2.0, 2, 2, 2 ** 64 - 1, 1]
    assert np.array_equal(rd(a[4], (P, 2)), REIM3[0]) and rd(a[5], (2,)).tolist() == [1.0, 0.5] and out.tolist() == [[0, 1, 2], [3, 4, 5]]
    fake.on["carma_simulate_carma"] = lambda *a: 1
    with pytest.raises(L.CarmaError) as e:
        L.simulate_carma(T5, 2.0, ROOTS, MA3[0])
    assert str(e.value) == "carma_process: repeated AR root (singular eigenvector matrix)"
    fake.on["carma_simulate_car1"] = lambda *a: (fill(a[6], (1, 3)), 0)[1]
    out = L.simulate_car1([3.0, 1.0, 2.0], 2.0, 0.25, seed=2 ** 64 + 5)
    a = fake.args("carma_simulate_car1")
    assert rd(a[0], (3,)).tolist() == [1.0, 2.0, 3.0] and [val(v) for v in a[1:6]] == [3, 2.0, 0.25, 1, 5] and val(a[7]) == 0
    assert out.tolist() == [[0, 1, 2]]


COND = [("carma", lambda **kw: L.simulate_cond_carma(T5, Y5, E5, SIG3, ROOTS3, MA3, kw.pop("mu", None), [9.0, 8.0], **kw), 6),
        ("car1", lambda **kw: L.simulate_cond_car1(T5, Y5, E5, SIG3, [0.5, 0.25, 0.125], kw.pop("mu", None), [9.0, 8.0], **kw), 3)]


@pytest.mark.parametrize("kind,call,nmodel", COND, ids=[c[0] for c in COND])
@pytest.mark.parametrize("parts", [False, True])
@pytest.mark.parametrize("flags", [False, True])
def test_simulate_cond(fake, kind, call, nmodel, parts, flags):
    K, M, m = 3, 2, 4                                           # m = n_out < n: rows come back to back
    cname = "carma_simulate_cond_" + kind
    seen = {}

    def sim(*a):
        seen["a"] = a
        mu, tp, Mq, seed, path0, out, unc, noi, sing, nout, dev = a[4 + nmodel:]
        fill(out, (K, M))
        assert null(unc) == null(noi) == (not parts)
        if parts:
            fill(unc, (K * (N + M),), 100), fill(noi, (K * N,), 200)
        wr(sing, seen.get("flags", [0, 0, 0]), np.int32), setref(nout, m)
        return 0
    fake.on[cname] = sim
    res = call(seed=-1, path0=2 ** 32 + 3, return_parts=parts, return_singular=flags, device=1, mu=[1.0, 2.0, 3.0])
    a = seen["a"]
    assert [rd(a[i], (N,)).tolist() for i in range(3)] == [T5.tolist(), Y5.tolist(), E5.tolist()] and val(a[3]) == N
    if kind == "carma":
        assert [val(a[4]), val(a[5]), val(a[9])] == [P, K, 2]
        assert np.array_equal(rd(a[6], (K,)), SIG3) and np.array_equal(rd(a[7], (K, P, 2)), REIM3) and np.array_equal(rd(a[8], (K, 2)), MA3)
    else:
        assert val(a[4]) == K and np.array_equal(rd(a[5], (K,)), SIG3) and rd(a[6], (K,)).tolist() == [0.5, 0.25, 0.125]
    mu, tp, Mq, seed, path0 = a[4 + nmodel:9 + nmodel]
    assert rd(mu, (K,)).tolist() == [1.0, 2.0, 3.0] and rd(tp, (M,)).tolist() == [9.0, 8.0]
    assert [val(Mq), val(seed), val(path0), val(a[-1])] == [M, 2 ** 64 - 1, 3, 1]
    res = res if isinstance(res, tuple) else (res,)
    assert len(res) == 1 + 3 * parts + flags
    assert np.array_equal(res[0], np.arange(6.0).reshape(K, M))
    if parts:
        assert np.array_equal(res[1], 100 + np.arange(1.0 * K * (m + M)).reshape(K, m + M))
        assert np.array_equal(res[2], 200 + np.arange(1.0 * K * m).reshape(K, m))
        assert res[3].tolist() == [0, 1, 2, 3, 4, 8, 9]
    if flags:
        assert res[-1].dtype == bool and res[-1].tolist() == [False] * 3
    call(return_parts=parts, return_singular=flags)             # mu None: NULL
    assert null(seen["a"][4 + nmodel]) and val(seen["a"][-1]) == 0 and val(seen["a"][7 + nmodel]) == 0
    seen["flags"] = [0, 1, 1]
    if flags:
        assert call(return_parts=parts, return_singular=True)[-1].tolist() == [False, True, True]
    else:
        with pytest.raises(L.CarmaError) as e:
            call(return_parts=parts)
        assert str(e.value) == "%s: repeated AR root (singular eigenvector matrix) in path 1" % cname
    with pytest.raises(ValueError) as e:
        call(mu=[1.0, 2.0])
    assert str(e.value) == "%s: mu must have one entry per path" % cname


def test_simulate_cond_model_count_errors(fake):
    for args in ((SIG3[:2], ROOTS3, MA3), (SIG3, ROOTS3, MA3[:2])):
        with pytest.raises(ValueError) as e:
            L.simulate_cond_carma(T5, Y5, E5, *args, None, [9.0])
        assert str(e.value) == "simulate_cond_carma: sigsqr, omega and ma must describe the same number of paths"
    with pytest.raises(ValueError) as e:
        L.simulate_cond_car1(T5, Y5, E5, SIG3, [0.5, 0.25], None, [9.0])
    assert str(e.value) == "simulate_cond_car1: sigsqr and omega must describe the same number of paths"
    for args in ((SIG3[:2], ROOTS3, MA3), (SIG3, ROOTS3, MA3[:2])):
        with pytest.raises(ValueError) as e:
            L.smooth_carma(T5, Y5, E5, *args, None, [9.0])
        assert str(e.value) == "smooth_carma: sigsqr, omega and ma must describe the same number of models"
    with pytest.raises(ValueError) as e:
        L.smooth_car1(T5, Y5, E5, SIG3, [0.5, 0.25], None, [9.0])
    assert str(e.value) == "smooth_car1: sigsqr and omega must describe the same number of models"
    assert not [n for n, _ in fake.calls if "cond" in n or "smooth" in n]


SMOOTH = [("carma", lambda **kw: L.smooth_carma(T5, Y5, E5, SIG3, ROOTS3, MA3, kw.pop("mu", None), [9.0, 8.0], **kw), 6),
          ("car1", lambda **kw: L.smooth_car1(T5, Y5, E5, SIG3, [0.5, 0.25, 0.125], kw.pop("mu", None), [9.0, 8.0], **kw), 3)]


@pytest.mark.parametrize("kind,call,nmodel", SMOOTH, ids=[c[0] for c in SMOOTH])
@pytest.mark.parametrize("band", [False, True, "only"])
@pytest.mark.parametrize("flags", [False, True])
def test_smooth(fake, kind, call, nmodel, band, flags):
    K, M = 3, 2
    cname = "carma_smooth_" + kind
    seen = {}

    def sm(*a):
        seen["a"] = a
        mu, tp, Mq, mean, var, bm, bv, sing, nout, dev = a[4 + nmodel:]
        assert null(mean) == null(var) == (band == "only") and null(bm) == null(bv) == (band is False)
        if band != "only":
            fill(mean, (K, M)), fill(var, (K, M), 10)
        if band:
            fill(bm, (M,), 20), fill(bv, (M,), 30)
        wr(sing, seen.get("flags", [0, 0, 0]), np.int32), setref(nout, 4)
        return 0
    fake.on[cname] = sm
    res = call(band=band, return_singular=flags, device=1, mu=[1.0, 2.0, 3.0])
    a = seen["a"]
    assert [rd(a[i], (N,)).tolist() for i in range(3)] == [T5.tolist(), Y5.tolist(), E5.tolist()] and val(a[3]) == N
    if kind == "carma":
        assert [val(a[4]), val(a[5]), val(a[9])] == [P, K, 2]
        assert np.array_equal(rd(a[6], (K,)), SIG3) and np.array_equal(rd(a[7], (K, P, 2)), REIM3) and np.array_equal(rd(a[8], (K, 2)), MA3)
    else:
        assert val(a[4]) == K and np.array_equal(rd(a[5], (K,)), SIG3) and rd(a[6], (K,)).tolist() == [0.5, 0.25, 0.125]
    assert rd(a[4 + nmodel], (K,)).tolist() == [1.0, 2.0, 3.0] and rd(a[5 + nmodel], (M,)).tolist() == [9.0, 8.0]
    assert val(a[6 + nmodel]) == M and val(a[-1]) == 1
    assert isinstance(res, tuple) and len(res) == 2 * (band != "only") + 2 * bool(band) + flags
    res = list(res)
    if band != "only":
        assert np.array_equal(res.pop(0), np.arange(6.0).reshape(K, M)) and np.array_equal(res.pop(0), 10 + np.arange(6.0).reshape(K, M))
    if band:
        assert res.pop(0).tolist() == [20, 21] and res.pop(0).tolist() == [30, 31]
    if flags:
        assert res[0].dtype == bool and res.pop(0).tolist() == [False] * 3
    assert not res
    call(band=band, return_singular=flags)
    assert null(seen["a"][4 + nmodel]) and val(seen["a"][-1]) == 0
    seen["flags"] = [0, 0, 1]
    if flags:
        assert call(band=band, return_singular=True)[-1].tolist() == [False, False, True]
    else:
        with pytest.raises(L.CarmaError) as e:
            call(band=band)
        assert str(e.value) == "%s: repeated AR root (singular eigenvector matrix) in model 2" % cname
    with pytest.raises(ValueError) as e:
        call(band=band, mu=[1.0])
    assert str(e.value) == "%s: mu must have one entry per model" % cname
    with pytest.raises(ValueError) as e:
        call(band="both")
    assert str(e.value) == "%s: band must be False, True or 'only'" % cname


def test_post_processing(fake):
    ns, nf = 3, 4
    fake.on["carma_sigma_noise_batch"] = lambda *a: (fill(a[6], (ns,), 5), 0)[1]
    out = L.sigma_noise_batch(ROOTS3, MA3, [1.0, 2.0, 3.0], device=1)
    a = fake.args("carma_sigma_noise_batch")
    assert [val(a[i]) for i in (0, 1, 5, 7)] == [P, 2, ns, 1] and np.array_equal(rd(a[2], (ns, P, 2)), REIM3)
    assert np.array_equal(rd(a[3], (ns, 2)), MA3) and rd(a[4], (ns,)).tolist() == [1.0, 2.0, 3.0] and out.tolist() == [5, 6, 7]
    with pytest.raises(ValueError, match="sigma_noise_batch: one row of roots, MA coefficients and one variance per sample"):
        L.sigma_noise_batch(ROOTS3, MA3[:2], [1.0, 2.0, 3.0])
    ar = np.arange(1.0, 1 + ns * (P + 1)).reshape(ns, P + 1)
    freq, perc = [0.1, 0.2, 0.3, 0.4], [16.0, 50.0]

    def psd(*a):
        fill(a[10], (nf, 2))
        if not null(a[11]):
            fill(a[11], (nf, ns), 100)
        return 0
    fake.on["carma_psd_band"] = psd
    band = L.psd_band(ar, MA3, SIG3, freq, perc)
    a = fake.args("carma_psd_band")
    assert [val(a[i]) for i in (0, 1, 5, 7, 9, 12)] == [P + 1, 2, ns, nf, 2, 0] and null(a[11])
    assert np.array_equal(rd(a[2], ar.shape), ar) and np.array_equal(rd(a[3], MA3.shape), MA3) and np.array_equal(rd(a[4], (ns,)), SIG3)
    assert rd(a[6], (nf,)).tolist() == freq and rd(a[8], (2,)).tolist() == perc and np.array_equal(band, np.arange(8.0).reshape(nf, 2))
    band, grid = L.psd_band(ar, MA3, SIG3, freq, perc, return_samples=True, device=1)
    assert np.array_equal(band, np.arange(8.0).reshape(nf, 2)) and np.array_equal(grid, 100 + np.arange(12.0).reshape(nf, ns))
    assert val(fake.args("carma_psd_band")[12]) == 1
    with pytest.raises(ValueError, match="psd_band: one row of AR coefficients, MA coefficients and one sigma per sample"):
        L.psd_band(ar, MA3, SIG3[:2], freq, perc)
    fake.on.update(carma_mpsd_fused_max=lambda: 4096, carma_mpsd_freq_tile=lambda: 8)
    assert (L.mpsd_fused_max(), L.mpsd_freq_tile()) == (4096, 8)


def test_mpsd_band(fake):
    N_, S, nf = 3, 2, 4
    ar = np.arange(1.0, 1 + N_ * (P + 1)).reshape(N_, P + 1)
    fake.on["carma_mpsd_band"] = lambda *a: (fill(a[11], (S, nf, a[10])), 0)[1]
    band = L.mpsd_band(ar, MA3, SIG3, [0, 2, 3], [0.1, 0.2, 0.3, 0.4], [16.0, 84.0], device=1)
    a = fake.args("carma_mpsd_band")
    assert [val(a[i]) for i in (0, 1, 6, 8, 10, 12)] == [P + 1, 2, S, nf, 2, 1] and rd(a[5], (S + 1,), np.int64).tolist() == [0, 2, 3]
    assert np.array_equal(rd(a[2], ar.shape), ar) and np.array_equal(rd(a[3], MA3.shape), MA3) and np.array_equal(rd(a[4], (N_,)), SIG3)
    assert rd(a[7], (S, nf)).tolist() == [[0.1, 0.2, 0.3, 0.4]] * 2 and rd(a[9], (2,)).tolist() == [16.0, 84.0]      # freq is broadcast
    assert np.array_equal(band, np.arange(16.0).reshape(S, nf, 2))
    fr2 = np.arange(1.0, 9.0).reshape(S, nf)
    L.mpsd_band(ar, MA3, SIG3, [0, 2, 3], fr2, 50.0)
    a = fake.args("carma_mpsd_band")
    assert np.array_equal(rd(a[7], (S, nf)), fr2) and val(a[10]) == 1 and val(a[12]) == 0
    n = fake.count("carma_mpsd_band")
    ok = dict(ar_coefs=ar, ma_coefs=MA3, sigma=SIG3, sample_start=[0, 2, 3], freq=fr2, percentiles=[50.0])
    for change, msg in ((dict(ar_coefs=ar[None]), r"mpsd_band: ar_coefs and ma_coefs must be \[N, p \+ 1\] and \[N, nma\]"),
                        (dict(ma_coefs=MA3[None]), r"mpsd_band: ar_coefs and ma_coefs must be"),
                        (dict(ma_coefs=MA3[:2]), "mpsd_band: one row of AR coefficients, MA coefficients and one sigma per sample"),
                        (dict(sigma=SIG3[:2]), "mpsd_band: one row of AR coefficients"),
                        (dict(sample_start=[0]), r"mpsd_band: sample_start must be \[S \+ 1\], start at 0, increase strictly and end at N = 3"),
                        (dict(sample_start=[1, 3]), "mpsd_band: sample_start must be"), (dict(sample_start=[0, 2]), "mpsd_band: sample_start must be"),
                        (dict(sample_start=[0, 2, 2, 3]), "mpsd_band: sample_start must be"),
                        (dict(freq=fr2[:1]), r"mpsd_band: freq must be \[nf\] or \[2, nf\] with nf >= 1, got \(1, 4\)"),
                        (dict(freq=[]), "mpsd_band: freq must be"), (dict(freq=fr2[None]), "mpsd_band: freq must be"),
                        (dict(percentiles=[]), r"mpsd_band: 1 \.\.\. 4 percentiles, got 0"),
                        (dict(percentiles=[1, 2, 3, 4, 5]), r"mpsd_band: 1 \.\.\. 4 percentiles, got 5")):
        with pytest.raises(ValueError, match=msg):
            L.mpsd_band(**dict(ok, **change))
    assert fake.count("carma_mpsd_band") == n


def test_chain_diag(fake):
    fake.on["carma_chain_diag_dmax"] = lambda: 2
    widths = []

    def diag(x, G, R_, L_, w, tau, mean, sigma, status, rhat, dev):
        xs = rd(x, (G, R_, L_, w))
        widths.append((G, R_, L_, w, dev))
        wr(tau, xs[:, :, 0, :]), wr(mean, 2 * xs[:, :, 0, :]), wr(sigma, 3 * xs[:, :, 0, :])
        wr(status, np.broadcast_to(np.arange(w), (G, R_, w)), np.int32)
        if not null(rhat):
            wr(rhat, xs[:, 0, 1, :])
        return 0
    fake.on["carma_chain_diag"] = diag
    G, L_, d = 2, 3, 5
    x = np.arange(1.0 * G * R * L_ * d).reshape(G, R, L_, d)
    out = L.chain_diag(x, device=1)
    assert widths == [(G, R, L_, 2, 1), (G, R, L_, 2, 1), (G, R, L_, 1, 1)]
    assert np.array_equal(out["tau"], x[:, :, 0, :]) and np.array_equal(out["mean"], 2 * x[:, :, 0, :]) and np.array_equal(out["sigma"], 3 * x[:, :, 0, :])
    assert out["status"].dtype == np.int32 and np.array_equal(out["status"], np.broadcast_to([0, 1, 0, 1, 0], (G, R, d)))
    assert np.array_equal(out["rhat"], x[:, 0, 1, :])
    del widths[:]
    out = L.chain_diag(x[..., :2], rhat=False)                 # one slab, no R-hat
    assert widths == [(G, R, L_, 2, 0)] and out["rhat"] is None and np.array_equal(out["tau"], x[:, :, 0, :2])
    for xin, shape in ((x[0, 0, :, 0], (1, 1, L_, 1)), (x[0, 0], (1, 1, L_, d)), (x[0], (1, R, L_, d))):
        del widths[:]
        out = L.chain_diag(xin)
        assert [w[:3] for w in widths] == [shape[:3]] * len(widths) and sum(w[3] for w in widths) == shape[3]
        assert out["tau"].shape == (shape[0], shape[1], shape[3]) and out["rhat"].shape == (shape[0], shape[3])
        assert np.array_equal(out["tau"][0, 0], np.atleast_1d(xin.reshape(-1, L_, shape[3])[0, 0]))
    with pytest.raises(ValueError, match=r"chain_diag: x must be \[G, R, L, d\] .* got 5 axes"):
        L.chain_diag(x[None])
    with pytest.raises(ValueError, match=r"chain_diag: x has an empty axis: \(2, 2, 0, 5\)"):
        L.chain_diag(x[:, :, :0])
    fake.on["carma_chain_diag_kernel_ms"] = lambda: 1.5
    assert L.chain_diag_kernel_ms() == 1.5 and L.chain_diag_dmax() == 2


def test_normalize_roots_and_merged_times(fake):
    fake.on["carma_normalize_roots"] = lambda p, om, out: (wr(out, rd(om, (p, 2))[::-1]), 0)[1]
    out = L.normalize_roots(ROOTS)
    a = fake.args("carma_normalize_roots")
    assert val(a[0]) == P and np.array_equal(rd(a[1], (P, 2)), REIM3[0]) and np.array_equal(out, ROOTS[::-1]) and out.dtype == complex
    fake.on["carma_normalize_roots"] = lambda *a: -22
    with pytest.raises(ValueError) as e:
        L.normalize_roots(ROOTS[:2] + 1j)
    assert str(e.value) == "the AR roots must be real or come in complex-conjugate pairs"
    grid, dpos, spos = L.merged_times([2.0, 0.0, 1.0, 1.0], [1.0, 5.0, 0.5])
    assert grid.tolist() == [0.0, 0.5, 1.0, 1.0, 2.0, 5.0] and dpos.tolist() == [0, 2, 4] and spos.tolist() == [3, 5, 1]
    assert not [n for n, _ in fake.calls if n != "carma_normalize_roots"]
