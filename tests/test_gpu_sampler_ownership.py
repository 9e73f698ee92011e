"""GPU tests of who owns the samplers' device buffers (carma_pack_amd/csrc/carma_pt_state.h): a sampler re-created on a context
holds nothing of the one before it, chain state the caller bound stays the caller's, and the sample buffers regrow.  Everything is
compared bit for bit with a fresh context; the requests and releases themselves are counted without a GPU in
tests/test_hostmem_cpu.py.

One synthetic series of 40 points, p = 2, q = 1, 5 temperatures x 2 replicas, 20 iterations."""
import numpy as np
import pytest

from helpers import irregular_series

pytestmark = pytest.mark.gpu

P, Q, T, R, NITER, SEED = 2, 1, 5, 2, 20, 20261020


@pytest.fixture(scope="module")
def cpa():
    import carma_pack_amd
    assert carma_pack_amd._lib.lib.carma_device_count() >= 1, "no MI355X visible"
    return carma_pack_amd


def _series():
    t, y, yerr = irregular_series(40, seed=77)
    return t, y, yerr, 10.0 * np.sqrt(np.mean(y * y) - np.mean(y) ** 2)


def _context(cpa):
    t, y, yerr, ms = _series()
    return cpa.Context(t, y, yerr, P, Q, max_stdev=ms)


def _run(ctx, kern):
    """pt_create -> pt_start -> NITER iterations on ctx (CARMA_PT_KERNEL is set by the caller); chains and factors."""
    ctx.pt_create(T, R, adapt_iters=NITER, seed=SEED)
    assert ctx.pt_kernel() == kern
    ctx.pt_start(None)
    ctx.pt_iterate(NITER)
    th, lp = ctx.pt_get_chains()
    return np.array(th), np.array(lp), np.array(ctx.pt_get_factor())


_FRESH = {}


def _fresh(cpa, kern):
    """The same on a context of its own, once per kernel for the whole module."""
    if kern not in _FRESH:
        ctx = _context(cpa)
        _FRESH[kern] = _run(ctx, kern)
        ctx.close()
        assert np.isfinite(_FRESH[kern][1]).all()
    return _FRESH[kern]


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(a, b, err_msg="%s: array %d" % (what, k))


def test_a_recreated_sampler_holds_nothing_of_the_one_before(cpa, monkeypatch):
    """ladder, row, lane and ladder again on ONE context: every state has buffers the others lack (row: staging, abort flag, backup;
    lane: scratch and the flags about where the factors are), and each run is the fresh context's."""
    ctx = _context(cpa)
    for step, kern in enumerate(["ladder", "row", "lane", "ladder"]):
        monkeypatch.setenv("CARMA_PT_KERNEL", kern)
        _assert_same(_run(ctx, kern), _fresh(cpa, kern), "creation %d (%s)" % (step, kern))
    ctx.close()
    assert not np.array_equal(_fresh(cpa, "ladder")[0][:, 0], _fresh(cpa, "ladder")[0][:, T - 1])     # (the chains moved apart)


@pytest.mark.parametrize("kern", ["ladder", "lane"])
def test_bound_chain_state_outlives_the_sampler_and_the_context(cpa, kern, monkeypatch):
    """The chain state in torch tensors (pt_bind_state): the sampler works in them, and neither a new sampler on the context nor
    the end of the context touches or releases them."""
    import torch
    monkeypatch.setenv("CARMA_PT_KERNEL", kern)
    ctx = _context(cpa)
    ctx.pt_create(T, R, adapt_iters=NITER, seed=SEED)
    th = torch.full((R, T, ctx.d), -1.0, dtype=torch.float64, device="cuda")
    lp = torch.full((R, T), -1.0, dtype=torch.float64, device="cuda")
    ctx.pt_bind_state(th.data_ptr(), lp.data_ptr())
    ctx.pt_start(None)
    ctx.pt_iterate(5)
    torch.cuda.synchronize()
    th5, lp5 = th.cpu().numpy().copy(), lp.cpu().numpy().copy()
    _assert_same((th5, lp5), ctx.pt_get_chains(), "bound tensors after 5 iterations")
    assert np.isfinite(lp5).all() and not (th5 == -1.0).any()
    # a new sampler on the context: the tensors are nobody's but the caller's, and the new sampler starts from nothing
    _assert_same(_run(ctx, kern), _fresh(cpa, kern), "sampler re-created after a bound one")
    torch.cuda.synchronize()
    _assert_same((th.cpu().numpy(), lp.cpu().numpy()), (th5, lp5), "bound tensors after pt_create")
    ctx.close()
    torch.cuda.synchronize()
    _assert_same((th.cpu().numpy(), lp.cpu().numpy()), (th5, lp5), "bound tensors after close")
    th += 1.0                                                  # still the caller's to write
    torch.cuda.synchronize()
    np.testing.assert_array_equal(th.cpu().numpy(), th5 + 1.0)


def test_multi_series_sampler_recreated_with_other_run_counts(cpa):
    """MultiContext.pt_create with two runs, then one, then three on one context: each is a fresh context's."""
    t, y, yerr, ms = _series()

    def run(mc, nruns):
        mc.pt_create([0] * nruns, T, R, NITER, seed=SEED)
        mc.pt_start(None)
        mc.pt_iterate(NITER)
        th, lp = mc.pt_get_chains()
        return np.array(th), np.array(lp), np.array(mc.pt_get_factor())

    mc = cpa.MultiContext([(t, y, yerr)], P, Q, max_stdev=[ms])
    for nruns in (2, 1, 3):
        fresh = cpa.MultiContext([(t, y, yerr)], P, Q, max_stdev=[ms])
        want = run(fresh, nruns)
        fresh.close()
        got = run(mc, nruns)
        assert got[0].size == nruns * R * T * mc.d and np.isfinite(got[1]).all()
        _assert_same(got, want, "%d run(s)" % nruns)
    mc.close()


@pytest.mark.parametrize("kern", ["ladder", "lane"])
def test_sample_buffers_grow_after_they_shrank(cpa, kern, monkeypatch):
    """pt_sample of 8, 3 and 20 on one sampler: the second call uses the first one's buffers with a stride of its own, the third
    outgrows them.  Together they are the 31 samples one call gives from the same seed and chains."""
    monkeypatch.setenv("CARMA_PT_KERNEL", kern)
    thin = 2

    def sampler():
        ctx = _context(cpa)
        ctx.pt_create(T, R, adapt_iters=10 ** 6, seed=SEED)
        assert ctx.pt_kernel() == kern
        return ctx

    a, b = sampler(), sampler()
    a.pt_start(None)
    b.pt_set_chains(*a.pt_get_chains())
    parts = [a.pt_sample(n, thin=thin) for n in (8, 3, 20)]
    s31, l31 = b.pt_sample(31, thin=thin)
    assert [p[0].shape for p in parts] == [(R, 8, a.d), (R, 3, a.d), (R, 20, a.d)] and parts[2][1].shape == (R, 20)
    np.testing.assert_array_equal(np.concatenate([p[0] for p in parts], axis=1), s31)
    np.testing.assert_array_equal(np.concatenate([p[1] for p in parts], axis=1), l31)
    assert np.isfinite(l31).all() and not np.array_equal(s31[:, 0], s31[:, 30])
    _assert_same(a.pt_get_chains(), b.pt_get_chains(), "chains after the sampling calls")
    a.close()
    b.close()
