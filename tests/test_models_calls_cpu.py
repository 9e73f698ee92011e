"""CPU-only: what the four model classes of carma_pack_amd/carma_pack.py (CarmaModel, CarmaModelSet, CarmaBandsModel,
CarmaBandsSet) ask of the C ABI and what they make of the answers -- every method that reaches a context, over the recording
library of fakelib.py.  Each test holds the sequence of C calls, their scalar arguments, the arrays behind their pointers and
what the method returns.

The scripted library (`World`) hands out a handle per create call and remembers the sizes behind it; output pointers are filled
with ramps (start + 0.01 i, in C order), so a wrong reshape, order or inverse permutation shows; integer outputs count up.  Shapes,
the smallest that can still go wrong: two series of 4 and 6 data and two objects of K = 2 bands with 10 and 12 data in all, so that
"longest first" reorders them and the inverse puts them back; ntrials = 2, nreplicas = 2, nsamples = 3.  No device, no library."""
import gc

import numpy as np
import pytest

import carma_pack_amd as cpa
import carma_pack_amd._lib as L
from fakelib import H, FakeLib, fill, null, rd, val, wr

TA, YA, EA = np.array([0.0, 1.0, 2.5, 4.0]), np.array([1.0, 3.0, 2.0, 5.0]), np.full(4, 0.1)
TB, YB, EB = 1.5 * np.arange(6.0), np.array([2.0, 1.0, 4.0, 3.0, 6.0, 5.0]), np.full(6, 0.2)
SERIES = [(TA, YA, EA), (TB, YB, EB)]                         # longest first: 1, 0
OBJECTS = [[SERIES[0], SERIES[1]], [(TB + 0.5, 2.0 * YB, EB), (TB + 1.0, YB + 1.0, EB)]]      # 10 and 12 data: longest first 1, 0
LAGB = [(-2.0, 3.0)]
NT, NR, NS, NTEMP, SEED = 2, 2, 3, 3, 5
FTOL = 2.220446049250313e-09
QUIET = ("carma_last_error", "carma_device_count", "carma_chain_diag_dmax")
ACCESSORS = ("_n", "_dim", "_nseries", "_nbands", "_nobjects", "_destroy")


def dim(p, q):
    return 4 if p == 1 else 3 + p + q


def ramp(shape, start=0.0, step=0.01):
    return start + step * np.arange(int(np.prod(shape))).reshape(shape)


def pop_max_stdev(y):
    return 10.0 * np.sqrt(np.mean(y * y) - np.mean(y) ** 2)


class World:
    """The scripted library: a handle per create call (`made`: handle -> what it holds), ramps into every output, the arguments
    of every call kept by fakelib.  `fun` scripts the optimiser's objective values: a function of the number of starts."""

    def __init__(self, fake):
        self.fake, self.made, self.lead = fake, {}, {}
        self.fun = lambda B: 50.0 - np.arange(B)
        self.invalid = None
        for name in dir(self):
            if name.startswith("carma_"):
                fake.on[name] = getattr(self, name)

    def _new(self, **info):
        h = H + 8 * len(self.made)
        self.made[h] = info
        return h

    def kinds(self):
        return [v["kind"] for v in self.made.values()]

    # ---- create and the accessors ----
    def carma_ctx_create(self, t, y, e, n, p, q, ms, dev):
        return self._new(kind="ctx", n=n, d=dim(p, q), t=rd(t, (n,)), y=rd(y, (n,)), e=rd(e, (n,)), p=p, q=q, ms=ms)

    def carma_ctx_n(self, h):
        return self.made[h]["n"]

    def carma_ctx_dim(self, h):
        return self.made[h]["d"]

    def _many(self, kind, t, y, e, off, nser, p, q, **more):
        off = rd(off, (nser + 1,), np.int64)
        cols = [rd(a, (off[-1],)) for a in (t, y, e)]
        return self._new(kind=kind, off=off.tolist(), n=np.diff(off), t=cols[0], y=cols[1], e=cols[2], p=p, q=q, **more)

    def carma_mctx_create(self, t, y, e, off, S, p, q, ms, dev):
        return self._many("mctx", t, y, e, off, S, p, q, d=dim(p, q), S=S, ms=rd(ms, (S,)).tolist())

    def carma_mctx_nseries(self, h):
        return self.made[h]["S"]

    def carma_mctx_dim(self, h):
        return self.made[h]["d"]

    def carma_mctx_n(self, h, s):
        return int(self.made[h]["n"][s])

    def carma_bands_create(self, t, y, e, off, K, p, q, lo, hi, ms, dev):
        return self._many("bands", t, y, e, off, K, p, q, d=3 + p + q + 3 * (K - 1), K=K, ms=ms,
                          lag=[rd(lo, (K - 1,)).tolist(), rd(hi, (K - 1,)).tolist()])

    def carma_bands_nbands(self, h):
        return self.made[h]["K"]

    def carma_bands_dim(self, h):
        return self.made[h]["d"]

    def carma_bands_n(self, h, b):
        return int(self.made[h]["n"][b])

    def carma_bandset_create(self, t, y, e, off, S, K, p, q, lo, hi, ms, dev):
        return self._many("bandset", t, y, e, off, S * K, p, q, d=3 + p + q + 3 * (K - 1), S=S, K=K, ms=rd(ms, (S,)).tolist(),
                          lag=[rd(lo, (S, K - 1)).tolist(), rd(hi, (S, K - 1)).tolist()])

    def carma_bandset_nobjects(self, h):
        return self.made[h]["S"]

    def carma_bandset_nbands(self, h):
        return self.made[h]["K"]

    def carma_bandset_dim(self, h):
        return self.made[h]["d"]

    def carma_bandset_n(self, h, s, b):
        return int(self.made[h]["n"][s * self.made[h]["K"] + b])

    # ---- log-densities: 100, 101, ... ----
    def carma_logdensity_batch(self, h, th, B, ip, out):
        fill(out, (B,), 100)
        return 0

    def carma_mlogdensity_batch(self, h, th, w, B, ip, out):
        fill(out, (B,), 100)
        return 0

    carma_bandset_logdensity_batch = carma_mlogdensity_batch
    carma_bands_logdensity_batch = carma_logdensity_batch

    # ---- the optimiser: x = x0 + 1, fun scripted, nit 1 ..., nfev 11 ..., status 0, 1, 2, 0, ... ----
    def _mle(self, a, nlead):
        B = a[3] if nlead == 7 or (nlead == 6 and self.made[a[0]]["kind"] == "mctx") else a[2]
        d = self.made[a[0]]["d"]
        x, fun, nit, nfev, status = a[nlead + 6:]
        wr(x, rd(a[1], (B, d)) + 1.0), wr(fun, self.fun(B)), fill(nit, (B,), 1, np.int32), fill(nfev, (B,), 11, np.int32)
        wr(status, np.arange(B) % 3, np.int32)
        return 0

    def carma_mle_batched(self, *a):
        return self._mle(a, 5)

    def carma_mle_batched_ms(self, *a):
        return self._mle(a, 6)

    def carma_bands_mle_batched(self, *a):
        return self._mle(a, 6)

    def carma_bandset_mle_batched(self, *a):
        return self._mle(a, 7)

    # ---- the samplers: samples 0.1 + 0.01 i, log-posteriors -5 + 0.01 i, acceptance rates 0.01 i, swap rates 0.5 + 0.01 i ----
    def _run(self, h, lead, S, samples, logposts):
        d = self.made[h]["d"]
        self.lead[h] = lead
        wr(samples, ramp(lead[:-1] + (S, d), 0.1)), wr(logposts, ramp(lead[:-1] + (S,), -5.0))
        return 0

    def _stats(self, h, acc, swp, reset):
        wr(acc, ramp(self.lead[h])), wr(swp, ramp(self.lead[h], 0.5))
        return 0

    carma_pt_stats = carma_mpt_stats = carma_bands_pt_stats = carma_bandset_pt_stats = _stats

    def carma_pt_run(self, h, T, R, S, burn, thin, init, ninit, seed, samples, logposts):
        return self._run(h, (R, T), S, samples, logposts)

    def carma_mpt_run(self, h, w, M, T, R, S, burn, thin, init, seed, samples, logposts):
        return self._run(h, (M, R, T), S, samples, logposts)

    def carma_bands_pt_run(self, h, T, R, S, burn, thin, init, seed, lo, hi, samples, logposts):
        return self._run(h, (R, T), S, samples, logposts)

    def carma_bandset_pt_run(self, h, w, M, T, R, S, burn, thin, init, seed, lo, hi, samples, logposts):
        return self._run(h, (M, R, T), S, samples, logposts)

    def carma_bands_pt_default_box(self, h, lo, hi):
        K = self.made[h]["K"]
        wr(lo, ramp((K - 1, 2), -7.0)), wr(hi, ramp((K - 1, 2), 7.0))
        return 0

    def carma_bandset_pt_default_box(self, h, s, lo, hi):
        K = self.made[h]["K"]
        wr(lo, ramp((K - 1, 2), -7.0 - s)), wr(hi, ramp((K - 1, 2), 7.0 + s))
        return 0

    # ---- filters and smoothers: means 0.01 i, variances 1 + 0.01 i ----
    def carma_mkfilter(self, h, w, M, sig, om, ma, nma, mu, mean, var, off, sing):
        ntot = int(self.made[h]["n"][rd(w, (M,), np.int32)].sum())
        wr(mean, ramp((ntot,))), wr(var, ramp((ntot,), 1.0))
        return 0

    def _at_times(self, h, w, M, sig, om, ma, nma, mu, tp, toff, pm, pv, sing):
        ntot = max(int(rd(toff, (M + 1,), np.int64)[-1]), 1)
        wr(pm, ramp((ntot,))), wr(pv, ramp((ntot,), 1.0))
        return 0

    carma_mpredict = carma_msmooth = _at_times

    def carma_bands_smooth(self, h, th, B, band, tp, M, mean, var, bm, bv, inv):
        wr(mean, ramp((B, M), 10.0 * band)), wr(var, ramp((B, M), 1.0))
        if not null(bm):
            wr(bm, ramp((M,), 20.0)), wr(bv, ramp((M,), 30.0))
        if self.invalid is not None:
            wr(inv, self.invalid, np.int32)
        return 0

    def carma_bandset_smooth(self, h, th, w, bo, B, tp, toff, mean, var, inv):
        ntot = max(int(rd(toff, (B + 1,), np.int64)[-1]), 1)
        wr(mean, ramp((ntot,))), wr(var, ramp((ntot,), 1.0))
        if self.invalid is not None:
            wr(inv, self.invalid, np.int32)
        return 0

    # ---- post-processing ----
    def carma_sigma_noise_batch(self, p, nma, om, ma, v, ns, out, dev):
        wr(out, ramp((ns,), 0.5))
        return 0

    def carma_mpsd_band(self, na, nma, ar, ma, sg, st, S, fr, nf, pc, npc, band, dev):
        wr(band, ramp((S, nf, npc)))
        return 0

    def carma_chain_diag_dmax(self):
        return 64

    def carma_chain_diag(self, x, G, R, Ln, d, tau, mean, sigma, status, rhat, dev):
        wr(tau, ramp((G, R, d), 2.0)), wr(mean, ramp((G, R, d), 3.0)), wr(sigma, ramp((G, R, d), 4.0))
        wr(status, np.zeros((G, R, d)), np.int32)
        if not null(rhat):
            wr(rhat, ramp((G, d), 1.0))
        return 0


@pytest.fixture
def fake(monkeypatch):
    f = FakeLib()
    monkeypatch.setattr(L, "lib", f)
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    f.world = World(f)
    yield f
    # an object a traceback still holds is released after the real library is back: it must not hand that one a scripted handle
    for o in gc.get_objects():
        if type(o) in (L.Context, L.MultiContext, L.BandsContext, L.BandsSetContext) and getattr(o, "_h", None) in f.world.made:
            o._h = None


def names(fake, since=0):
    """The C calls so far, in order, without the accessors, the releases and the calls that ask the library about itself."""
    return [n for n, _ in fake.calls[since:] if n not in QUIET and not n.endswith(ACCESSORS)]


def mark(fake):
    return len(fake.calls)


def scalars(a, idx):
    return [val(a[i]) for i in idx]


# ---- what the classes compute on the host, written out once more ------------------------------------------
def ref_bounds(t, y, p, q):
    ysigma, dt = y.std(), np.diff(t)
    max_freq, min_freq = 0.9 / dt.min(), 1.0 / (t.max() - t.min())
    b = [(ysigma / 10.0, 10.0 * ysigma), (0.9, 1.1), (None, None)]
    if p == 1:
        return b + [(np.log(min_freq), np.log(max_freq))]
    return b + [(np.log(min(min_freq ** 2, 2.0 * min_freq)), np.log(max(max_freq ** 2, 2.0 * max_freq)))] * p + [(None, None)] * q


def ref_lohi(bnds, extra=0):
    return (np.array([-np.inf if b[0] is None else b[0] for b in bnds] + [-np.inf] * extra),
            np.array([np.inf if b[1] is None else b[1] for b in bnds] + [np.inf] * extra))


def ref_starts(raw, bnds, seed):
    """A sampler's draws raw [ntrials, d] -> the starts: error scale 1, whatever lies outside its box drawn anew, column by column."""
    st, rng = raw.copy(), np.random.default_rng(seed)
    st[:, 1] = 1.0
    for j, (lo, hi) in enumerate(bnds):
        if lo is not None:
            out = (st[:, j] < lo) | (st[:, j] > hi)
            st[out, j] = rng.uniform(lo, hi, int(out.sum()))
    return st


def ref_band_starts(bands, st, lagb, seed):
    d, K = st.shape[1], len(bands)
    x0, rng, s0 = np.empty((st.shape[0], d + 3 * (K - 1))), np.random.default_rng(seed), bands[0][1].std()
    x0[:, :d] = st
    for b in range(1, K):
        c = d + 3 * (b - 1)
        x0[:, c] = rng.uniform(lagb[b - 1][0], lagb[b - 1][1], st.shape[0])
        x0[:, c + 1], x0[:, c + 2] = np.log(bands[b][1].std() / s0), bands[b][1].mean()
    return x0


def raw_draws(ntrials, d):
    """What the scripted carma_pt_run hands _mle_problem: the one sample of each of ntrials replicas."""
    return ramp((ntrials, 1, d), 0.1)[:, 0, :]


def object_starts(bands, p, q, ntrials, seed):
    """(x0, lo, hi) of a multi-band object: band 0's CarmaModel starts, then the band columns."""
    bnds = ref_bounds(bands[0][0], bands[0][1], p, q)
    lo, hi = ref_lohi(bnds, 3 * (len(bands) - 1))
    return ref_band_starts(bands, ref_starts(raw_draws(ntrials, dim(p, q)), bnds, seed), LAGB, seed), lo, hi


def check_fit(r, x, fun, i):
    assert isinstance(r, cpa.carma_pack.BatchResult) and np.array_equal(r.x, x) and r.fun == fun
    assert (r.nit, r.nfev, r.success, r.message) == (1 + i, 11 + i, i % 3 < 2, cpa.carma_pack.STATUS_TEXT[i % 3])


def check_start_sampler(fake, h, t, y, p, q, seed, k=-1):
    """The short tempered run that draws the starts of one series: its context, its prior bound and its sampler call."""
    made = fake.world.made[h]
    assert made["kind"] == "ctx" and (made["p"], made["q"]) == (p, q) and np.array_equal(made["t"], t) and np.array_equal(made["y"], y)
    assert made["ms"] == 10.0 * np.sqrt(np.var(y, ddof=1))
    sp = [a for n, a in fake.calls if n == "carma_ctx_set_prior" and a[0] == h]
    assert len(sp) == 1 and sp[0][1] == pop_max_stdev(y)
    a = [a for n, a in fake.calls if n == "carma_pt_run" and a[0] == h][k]
    assert scalars(a, range(1, 6)) == [1 if p == 1 else 10, NT, 1, 25, 1] and null(a[6]) and val(a[7]) == 0 and val(a[8]) == seed


# ---- CarmaModel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q", [(1, 0), (2, 1)])
def test_carmamodel_mle_problem_and_get_mle(fake, p, q):
    d = dim(p, q)
    m = cpa.CarmaModel(TA, YA, EA, p=p, q=q)
    proc, starts, bnds = m._mle_problem(p, q, NT, SEED)
    assert names(fake) == ["carma_ctx_create", "carma_ctx_set_prior", "carma_pt_run", "carma_pt_stats"]
    check_start_sampler(fake, H, TA, YA, p, q, SEED)
    assert bnds == ref_bounds(TA, YA, p, q) == m._mle_bounds(p, q)
    want = ref_starts(raw_draws(NT, d), bnds, SEED)
    assert np.array_equal(starts, want) and not np.array_equal(starts[:, 0], raw_draws(NT, d)[:, 0])       # (a draw left its box)
    assert proc._ignore_prior == (p > 1)

    fake.world.fun = lambda B: np.array([np.inf, 7.0])[:B]
    k = mark(fake)
    best = m.get_mle(p, q, ntrials=NT, seed=SEED)
    assert names(fake, k) == ["carma_ctx_create", "carma_ctx_set_prior", "carma_pt_run", "carma_pt_stats", "carma_mle_batched"]
    a = fake.args("carma_mle_batched")
    lo, hi = ref_lohi(bnds)
    assert a[0] == H + 8 and np.array_equal(rd(a[1], (NT, d)), want) and val(a[2]) == NT
    assert np.array_equal(rd(a[3], (d,)), lo) and np.array_equal(rd(a[4], (d,)), hi)
    assert scalars(a, range(5, 11)) == [2000, 8, FTOL, 1e-5, 1e-6, int(p > 1)]
    check_fit(best, want[1] + 1.0, 7.0, 1)                                        # the best finite one
    fake.world.fun = lambda B: np.array([np.inf, np.inf])[:B]
    check_fit(m.get_mle(p, q, ntrials=NT, seed=SEED), want[0] + 1.0, np.inf, 0)    # none finite: the best of all, the first of equals
    fake.world.fun = lambda B: np.array([3.0, 7.0])[:B]
    every = m.get_mle(p, q, ntrials=NT, seed=SEED, return_all=True)
    assert len(every) == NT
    for i, r in enumerate(every):
        check_fit(r, want[i] + 1.0, [3.0, 7.0][i], i)
    with pytest.raises(ValueError, match="method must be 'batched' or 'scipy'"):
        m.get_mle(p, q, ntrials=NT, seed=SEED, method="nope")


# ---- CarmaModelSet ------------------------------------------------------------------------------------------
def check_mctx(fake, h, p, q):
    made = fake.world.made[h]
    assert made["kind"] == "mctx" and (made["p"], made["q"], made["S"], made["off"]) == (p, q, 2, [0, 4, 10])
    assert np.array_equal(made["t"], np.r_[TA, TB]) and np.array_equal(made["y"], np.r_[YA, YB]) and np.array_equal(made["e"], np.r_[EA, EB])
    assert made["ms"] == [pop_max_stdev(YA), pop_max_stdev(YB)]


def test_modelset_loglik(fake):
    ms = cpa.CarmaModelSet(SERIES, p=2, q=1)
    th = ramp((3, 6))
    out = ms.loglik(th, [1, 0, 1])
    assert names(fake) == ["carma_mctx_create", "carma_mlogdensity_batch"]
    check_mctx(fake, H, 2, 1)
    a = fake.args("carma_mlogdensity_batch")
    assert a[0] == H and np.array_equal(rd(a[1], (3, 6)), th) and rd(a[2], (3,), np.int32).tolist() == [1, 0, 1] and scalars(a, (3, 4)) == [3, 1]
    assert out.tolist() == [100.0, 101.0, 102.0]
    one = ms.loglik(th[2], 1)
    a = fake.args("carma_mlogdensity_batch")
    assert isinstance(one, float) and one == 100.0 and np.array_equal(rd(a[1], (1, 6)), th[2:]) and rd(a[2], (1,), np.int32).tolist() == [1]
    assert fake.count("carma_mctx_create") == 1                                  # the context is kept
    with pytest.raises(ValueError, match="series index out of range"):
        ms.loglik(th, 2)
    m1 = cpa.CarmaModelSet(SERIES, p=1)
    m1.loglik(ramp((2, 4)), 0)
    assert val(fake.args("carma_mlogdensity_batch")[4]) == 0                     # p = 1 has no SetMLE


def run_set(fake, p, q, **kw):
    ms = cpa.CarmaModelSet(SERIES, p=p, q=q)
    out = ms.run_mcmc(NS, ntemperatures=NTEMP, nreplicas=NR, seed=SEED, **kw)
    return ms, out


@pytest.mark.parametrize("p,q", [(1, 0), (2, 1)])
def test_modelset_run_mcmc(fake, p, q):
    d, T = dim(p, q), (NTEMP if p > 1 else 1)
    init = ramp((2, d), 0.3)
    ms, out = run_set(fake, p, q, init=init)
    assert names(fake) == ["carma_mctx_create", "carma_mpt_run", "carma_mpt_stats"] + (["carma_mlogdensity_batch", "carma_sigma_noise_batch"]
                                                                                   if p > 1 else [])
    check_mctx(fake, H, p, q)
    a = fake.args("carma_mpt_run")
    assert a[0] == H and rd(a[1], (2,), np.int32).tolist() == [1, 0] and scalars(a, range(2, 8)) == [2, T, NR, NS, NS // 2, 1]
    assert np.array_equal(rd(a[8], (2, d)), init[[1, 0]]) and val(a[9]) == SEED and val(fake.args("carma_mpt_stats")[3]) == 0
    samples, logposts = ramp((2, NR, NS, d), 0.1), ramp((2, NR, NS), -5.0)       # run j is series (1, 0)[j]
    acc, swp = ramp((2, NR, T)), ramp((2, NR, T), 0.5)
    if p > 1:
        a = fake.args("carma_mlogdensity_batch")
        assert np.array_equal(rd(a[1], (2 * NS, d)), samples[:, 0].reshape(-1, d)) and rd(a[2], (2 * NS,), np.int32).tolist() == [1] * NS + [0] * NS
        assert scalars(a, (3, 4)) == [2 * NS, 1]
        a = fake.args("carma_sigma_noise_batch")
        ins = [cpa.CarmaSample._sigma_inputs_of(samples[j, 0], p, q) for j in range(2)]
        assert scalars(a, (0, 1, 5)) == [p, q + 1, 2 * NS]
        roots = np.concatenate([i[0] for i in ins])
        assert np.array_equal(rd(a[2], (2 * NS, p, 2)), np.stack([roots.real, roots.imag], axis=-1))
        assert np.array_equal(rd(a[3], (2 * NS, q + 1)), np.concatenate([i[1] for i in ins]))
        assert np.array_equal(rd(a[4], (2 * NS,)), np.concatenate([i[2] for i in ins]))
    assert ms.mcmc_samples is out and len(out) == 2
    for j, s in enumerate((1, 0)):
        smp = out[s]
        assert type(smp) is (cpa.Car1Sample if p == 1 else cpa.CarmaSample) and ms.models[s].mcmc_sample is smp
        assert smp.time is ms.models[s].time and smp.y is ms.models[s].y
        every, lps = smp._sampler.getAllSamples()
        assert np.array_equal(every, samples[j]) and np.array_equal(lps, logposts[j]) and smp._sampler._series == s
        assert np.array_equal(smp._sampler.accept_rate, acc[j]) and np.array_equal(smp._sampler.swap_rate, swp[j])
        assert np.array_equal(smp._samples["logpost"][:, 0], logposts[j, 0]) and np.array_equal(smp._samples["mu"][:, 0], samples[j, 0, :, 2])
        if p > 1:
            assert np.array_equal(smp._samples["loglik"][:, 0], 100.0 + NS * j + np.arange(NS))
            assert np.array_equal(smp._samples["sigma"][:, 0], ramp((2 * NS,), 0.5)[j * NS:(j + 1) * NS])
    for kw, msg in ((dict(nsamples=0), "nsamples"), (dict(nthin=0), "nthin"), (dict(nreplicas=0), "nreplicas"),
                    (dict(ntemperatures=65), "ntemperatures"), (dict(ntemperatures=0), "ntemperatures"), (dict(nburnin=-1), "nburnin"),
                    (dict(init=init[0]), r"init must be \[2, %d\] \(one row per series\)" % d)):
        k = mark(fake)
        with pytest.raises(ValueError, match=msg):
            ms.run_mcmc(**dict(dict(nsamples=NS), **kw))
        assert names(fake, k) == []                                              # refused before any library call
    k = mark(fake)
    ms.run_mcmc(NS, seed=SEED)                                                   # the defaults: a ladder of max(10, p + q), no init
    a = fake.args("carma_mpt_run")
    assert scalars(a, range(2, 8)) == [2, 10 if p > 1 else 1, 1, NS, NS // 2, 1] and null(a[8]) and fake.count("carma_mctx_create") == 1


def test_modelset_power_spectrum_band_and_diagnostics(fake):
    p, q, d = 2, 1, 6
    ms, out = run_set(fake, p, q)
    k = mark(fake)
    lower, upper, median, freq = ms.power_spectrum_band(percentile=90.0, freq=[0.1, 0.2, 0.4, 0.8])
    assert names(fake, k) == ["carma_mpsd_band"]
    a = fake.args("carma_mpsd_band")
    assert scalars(a, (0, 1, 6, 8, 10)) == [p + 1, q + 1, 2, 4, 3] and rd(a[5], (3,), np.int64).tolist() == [0, NS, 2 * NS]
    assert np.array_equal(rd(a[2], (2 * NS, p + 1)), np.concatenate([s._samples["ar_coefs"] for s in out]))
    assert np.array_equal(rd(a[3], (2 * NS, q + 1)), np.concatenate([s._samples["ma_coefs"] for s in out]))
    assert np.array_equal(rd(a[4], (2 * NS,)), np.concatenate([s._samples["sigma"][:, 0] for s in out]))
    assert np.array_equal(rd(a[7], (2, 4)), np.tile([0.1, 0.2, 0.4, 0.8], (2, 1))) and rd(a[9], (3,)).tolist() == [5.0, 50.0, 95.0]
    band = ramp((2, 4, 3))
    assert np.array_equal(lower, band[:, :, 0]) and np.array_equal(upper, band[:, :, 2]) and np.array_equal(median, band[:, :, 1])
    assert np.array_equal(freq, np.tile([0.1, 0.2, 0.4, 0.8], (2, 1)))
    ms.power_spectrum_band(nsamples=2, samples=out[::-1])                        # each series' own grid, a subsample, the caller's samples
    a = fake.args("carma_mpsd_band")
    assert scalars(a, (6, 8)) == [2, 1000] and rd(a[5], (3,), np.int64).tolist() == [0, 2, 4]
    assert np.array_equal(rd(a[7], (2, 1000)), np.stack([s._psd_frequencies() for s in out[::-1]]))
    assert np.array_equal(rd(a[4], (4,)), np.concatenate([s._samples["sigma"][[0, 1], 0] for s in out[::-1]]))
    k = mark(fake)
    diag = ms.diagnostics()
    assert names(fake, k) == ["carma_chain_diag", "carma_chain_diag"]
    a, b = fake.args("carma_chain_diag", -2), fake.args("carma_chain_diag", -1)
    assert scalars(a, range(1, 5)) == [2, NR, NS, d] and scalars(b, range(1, 5)) == [2, NR, NS, 1]
    assert np.array_equal(rd(a[0], (2, NR, NS, d)), ramp((2, NR, NS, d), 0.1)[[1, 0]])                    # the caller's order
    assert np.array_equal(rd(b[0], (2, NR, NS, 1)), ramp((2, NR, NS), -5.0)[[1, 0]][..., None])
    for key, start in (("tau", 2.0), ("mean", 3.0), ("sigma", 4.0)):
        assert np.array_equal(diag[key], np.concatenate([ramp((2, NR, d), start), ramp((2, NR, 1), start)], axis=-1))
    assert np.array_equal(diag["rhat"], np.concatenate([ramp((2, d), 1.0), ramp((2, 1), 1.0)], axis=-1))
    assert np.array_equal(diag["ess"], np.sum(NS / diag["tau"], axis=1)) and diag["status"].shape == (2, NR, d + 1)
    fresh = cpa.CarmaModelSet(SERIES, p=p, q=q)
    for call in (fresh.power_spectrum_band, fresh.diagnostics):
        with pytest.raises(ValueError, match="no samples: call run_mcmc first, or pass samples="):
            call()
        with pytest.raises(ValueError, match=r"samples must hold one sample object per series \(2\), got 1"):
            call(samples=out[:1])


@pytest.mark.parametrize("p,q", [(1, 0), (2, 1)])
def test_modelset_get_mle(fake, p, q):
    d = dim(p, q)
    ms = cpa.CarmaModelSet(SERIES, p=p, q=q)
    bnds = [ref_bounds(t, y, p, q) for t, y, _ in SERIES]
    lo, hi = (np.stack(a) for a in zip(*[ref_lohi(b) for b in bnds]))
    fake.world.fun = lambda B: np.array([3.0, 2.0, np.inf, 9.0])[:B]

    def check_call(want):
        a = fake.args("carma_mle_batched_ms")
        assert np.array_equal(rd(a[1], (2 * NT, d)), want.reshape(2 * NT, d)) and rd(a[2], (2 * NT,), np.int32).tolist() == [0, 0, 1, 1]
        assert val(a[3]) == 2 * NT and np.array_equal(rd(a[4], (2 * NT, d)), lo[[0, 0, 1, 1]]) and np.array_equal(rd(a[5], (2 * NT, d)), hi[[0, 0, 1, 1]])
        assert scalars(a, range(6, 12)) == [2000, 8, FTOL, 1e-5, 1e-6, int(p > 1)]
        assert fake.world.made[a[0]]["kind"] == "mctx"

    # starts None: every series' own short run, in the caller's order, then one lock-step run
    fits = ms.get_mle(p, q, ntrials=NT, seed=SEED)
    assert names(fake) == ["carma_ctx_create", "carma_ctx_set_prior", "carma_pt_run", "carma_pt_stats"] * 2 + ["carma_mctx_create",
                                                                                                             "carma_mle_batched_ms"]
    for s, (t, y, _) in enumerate(SERIES):
        check_start_sampler(fake, H + 8 * s, t, y, p, q, SEED)
    check_mctx(fake, H + 16, p, q)
    want = np.stack([ref_starts(raw_draws(NT, d), b, SEED) for b in bnds])
    check_call(want)
    check_fit(fits[0], want[0, 1] + 1.0, 2.0, 1)
    check_fit(fits[1], want[1, 1] + 1.0, 9.0, 3)                                 # (start 2 is not finite)
    assert set(ms.timing) == {"starts_s", "optimise_s"} and all(v >= 0 for v in ms.timing.values())
    # "set": one multi-series run for all starts, longest series first, put back in the caller's order
    k = mark(fake)
    every = ms.get_mle(p, q, ntrials=NT, seed=SEED, starts="set", return_all=True)
    assert names(fake, k) == ["carma_mpt_run", "carma_mle_batched_ms"]
    a = fake.args("carma_mpt_run")
    assert rd(a[1], (2,), np.int32).tolist() == [1, 0] and scalars(a, range(2, 8)) == [2, 1 if p == 1 else 10, NT, 1, 25, 1]
    assert null(a[8]) and val(a[9]) == SEED
    raw = ramp((2, NT, 1, d), 0.1)[:, :, 0, :]                                   # run j is series (1, 0)[j]
    want = np.stack([ref_starts(raw[1], bnds[0], SEED), ref_starts(raw[0], bnds[1], SEED)])
    check_call(want)
    assert [len(e) for e in every] == [NT, NT]
    for i in range(2 * NT):
        check_fit(every[i // NT][i % NT], want[i // NT, i % NT] + 1.0, [3.0, 2.0, np.inf, 9.0][i], i)
    # an array: nothing is drawn
    k = mark(fake)
    given = ramp((2, NT, d), 0.7)
    fits = ms.get_mle(p, q, starts=given)
    assert names(fake, k) == ["carma_mle_batched_ms"]
    check_call(given)
    check_fit(fits[0], given[0, 1] + 1.0, 2.0, 1)
    for starts, msg in (("nope", "starts must be None, 'set' or an array"), (given[:1], r"starts must be \[2, ntrials, %d\]" % d),
                        (given[:, :, :3], r"starts must be \[2, ntrials, %d\]" % d)):
        with pytest.raises(ValueError, match=msg):
            ms.get_mle(p, q, starts=starts)


def test_modelset_choose_order(fake):
    longer = [(np.arange(7.0), np.r_[YB, 4.0], np.full(7, 0.2)), (1.5 * np.arange(9.0), np.r_[YA, YB[:5]], np.full(9, 0.1))]       # n > k + 1 at (2, 1)
    ms = cpa.CarmaModelSet(longer)
    shift = {4: 0.0, 5: -6.0, 6: -2.0}                         # the objective of an order, by its dimension: (2, 0) is the best fit
    fake.world.fun = lambda B: np.array([3.0, 2.0, 4.0, 9.0])[:B] + shift[fake.world.made[fake.calls[-1][1][0]]["d"]]
    out = ms.choose_order(2, ntrials=NT, seed=SEED)
    pqlist = [(1, 0), (2, 0), (2, 1)]
    assert names(fake) == (["carma_ctx_create", "carma_ctx_set_prior", "carma_pt_run", "carma_pt_stats"] * 2
                           + ["carma_mctx_create", "carma_mle_batched_ms"]) * 3
    assert [(v["p"], v["q"]) for v in fake.world.made.values() if v["kind"] == "mctx"] == pqlist
    for s, (n, fbest) in enumerate(((7, 2.0), (9, 4.0))):
        best, pq, aicc = out[s]
        want = []
        for p, q in pqlist:
            kk = 2 + p + q
            want.append(2.0 * kk + 2.0 * (fbest + shift[dim(p, q)]) + 2.0 * kk * (kk + 1.0) / (n - kk - 1.0))
        assert pq == pqlist and aicc == want
        i = int(np.argmin(want))
        assert ms.orders[s] == pqlist[i] and best.fun == fbest + shift[dim(*pqlist[i])] and best.x.size == dim(*pqlist[i])
    assert ms.orders == [(1, 0), (2, 0)]                       # (7 data: the penalty decides; 9 data: the fit does)
    with pytest.raises(ValueError, match="at least 1"):
        ms.choose_order(0)


FITS = [np.array([1.5, 1.0, 0.25, -1.0, 0.5, 0.3]), np.array([2.5, 1.0, -0.75, -0.5, 0.8, -0.2])]         # (2, 1) vectors


def check_items(a, idx):
    mods = [cpa.mle_to_model(FITS[s], 2, 1) for s in idx]
    M = len(idx)
    assert rd(a[1], (M,), np.int32).tolist() == list(idx) and val(a[2]) == M and rd(a[3], (M,)).tolist() == [m[0] for m in mods]
    roots = np.stack([m[1] for m in mods])
    assert np.array_equal(rd(a[4], (M, 2, 2)), np.stack([roots.real, roots.imag], axis=-1))
    assert np.array_equal(rd(a[5], (M, 2)), np.stack([m[2] for m in mods])) and val(a[6]) == 2 and rd(a[7], (M,)).tolist() == [m[3] for m in mods]


@pytest.mark.parametrize("method,cname", [("predict", "carma_mpredict"), ("smooth", "carma_msmooth")])
def test_modelset_predict_and_smooth(fake, method, cname):
    ms = cpa.CarmaModelSet(SERIES, p=2, q=1)
    mean, var = getattr(ms, method)([9.0, 8.0, 7.5], FITS)                       # one array for every series
    assert names(fake) == ["carma_mctx_create", cname]
    check_mctx(fake, H, 2, 1)
    a = fake.args(cname)
    check_items(a, (0, 1))
    assert rd(a[8], (6,)).tolist() == [9.0, 8.0, 7.5] * 2 and rd(a[9], (3,), np.int64).tolist() == [0, 3, 6]
    assert [m.tolist() for m in mean] == [ramp((3,)).tolist(), ramp((3,), 0.03).tolist()]
    assert [v.tolist() for v in var] == [ramp((3,), 1.0).tolist(), ramp((3,), 1.03).tolist()]

    class Fit:
        def __init__(self, x):
            self.x = x
    mean, var = getattr(ms, method)([[9.0], np.array([8.0, 7.5, 7.0])], [Fit(x) for x in FITS], orders=(2, 1))      # one per series
    a = fake.args(cname)
    check_items(a, (0, 1))
    assert rd(a[8], (4,)).tolist() == [9.0, 8.0, 7.5, 7.0] and rd(a[9], (3,), np.int64).tolist() == [0, 1, 4]
    assert [m.tolist() for m in mean] == [[0.0], [0.01, 0.02, 0.03]] and [v.tolist() for v in var] == [[1.0], [1.01, 1.02, 1.03]]
    # an order per series: one call per order present, the results back in the caller's order
    k = mark(fake)
    mean, var = getattr(ms, method)(4.5, [FITS[0][:5], FITS[1]], orders=[(2, 0), (2, 1)])
    assert names(fake, k) == ["carma_mctx_create", cname, cname]
    a, b = fake.args(cname, -2), fake.args(cname, -1)
    assert fake.world.made[a[0]]["q"] == 0 and a[0] != b[0] and b[0] == H
    assert rd(a[1], (1,), np.int32).tolist() == [0] and rd(b[1], (1,), np.int32).tolist() == [1] and rd(b[8], (1,)).tolist() == [4.5]
    assert [m.tolist() for m in mean] == [[0.0], [0.0]]
    with pytest.raises(ValueError, match=r"times must be one array, or one per series \(2\), got 3"):
        getattr(ms, method)([[1.0], [2.0], [3.0]], FITS)
    mean, var = getattr(ms, method)(np.array([[9.0, 8.0], [7.5, 7.0]]), FITS)     # an array [S, M]: a row of times per series
    a = fake.args(cname)
    assert rd(a[8], (4,)).tolist() == [9.0, 8.0, 7.5, 7.0] and rd(a[9], (3,), np.int64).tolist() == [0, 2, 4]
    assert [m.tolist() for m in mean] == [[0.0, 0.01], [0.02, 0.03]] and [v.shape for v in var] == [(2,), (2,)]
    with pytest.raises(ValueError, match=r"fits must hold one result per series \(2\), got 1"):
        getattr(ms, method)([1.0], FITS[:1])


def test_modelset_assess_fit(fake):
    ms = cpa.CarmaModelSet(SERIES, p=2, q=1)
    out = ms.assess_fit(FITS, nplot=5)
    assert names(fake) == ["carma_mctx_create", "carma_mkfilter", "carma_mpredict"]
    a = fake.args("carma_mkfilter")
    check_items(a, (0, 1))
    assert null(a[10])
    a = fake.args("carma_mpredict")
    check_items(a, (0, 1))
    grids = [np.linspace(t.min(), t.max(), 5) for t, _, _ in SERIES]
    assert np.array_equal(rd(a[8], (10,)), np.concatenate(grids)) and rd(a[9], (3,), np.int64).tolist() == [0, 5, 10]
    kmean, kvar = np.split(ramp((10,)), [4]), np.split(ramp((10,), 1.0), [4])
    for s, (t, y, _) in enumerate(SERIES):
        resid = (y - kmean[s]) / np.sqrt(kvar[s])
        r0 = resid - resid.mean()
        acf = np.correlate(r0, r0, mode="full")[r0.size - 1:]
        assert sorted(out[s]) == ["mean", "resid_acf", "std_resid", "time", "var"] and np.array_equal(out[s]["time"], grids[s])
        assert np.array_equal(out[s]["mean"], ramp((10,))[5 * s:5 * s + 5]) and np.array_equal(out[s]["var"], ramp((10,), 1.0)[5 * s:5 * s + 5])
        assert np.array_equal(out[s]["std_resid"], resid) and np.array_equal(out[s]["resid_acf"], acf / acf[0])


# ---- CarmaBandsModel ----------------------------------------------------------------------------------------
def check_bands(fake, h, bands, p, q):
    made = fake.world.made[h]
    n0 = bands[0][0].size
    assert made["kind"] == "bands" and (made["p"], made["q"], made["K"], made["off"]) == (p, q, 2, [0, n0, n0 + bands[1][0].size])
    for i, key in enumerate("tye"):
        assert np.array_equal(made[key], np.concatenate([b[i] for b in bands]))
    assert made["lag"] == [[-2.0], [3.0]] and made["ms"] == pop_max_stdev(bands[0][1])


def test_bandsmodel_loglik_logpost(fake):
    bm = cpa.CarmaBandsModel(OBJECTS[0], p=2, q=1, lag_bounds=LAGB)
    th = ramp((3, 9))
    assert bm.loglik(th).tolist() == [100.0, 101.0, 102.0]
    assert names(fake) == ["carma_bands_create", "carma_bands_logdensity_batch"]
    check_bands(fake, H, OBJECTS[0], 2, 1)
    a = fake.args("carma_bands_logdensity_batch")
    assert a[0] == H and np.array_equal(rd(a[1], (3, 9)), th) and scalars(a, (2, 3)) == [3, 1]
    one = bm.logpost(th[1])
    a = fake.args("carma_bands_logdensity_batch")
    assert isinstance(one, float) and one == 100.0 and np.array_equal(rd(a[1], (1, 9)), th[1:2]) and scalars(a, (2, 3)) == [1, 0]
    b1 = cpa.CarmaBandsModel(OBJECTS[0], p=1, lag_bounds=LAGB)
    b1.loglik(ramp((7,)))
    assert val(fake.args("carma_bands_logdensity_batch")[3]) == 0 and fake.count("carma_bands_create") == 2


@pytest.mark.parametrize("p,q", [(1, 0), (2, 1)])
def test_bandsmodel_get_mle_and_lag_profile(fake, p, q):
    d = dim(p, q)
    dx = d + 3
    bm = cpa.CarmaBandsModel(OBJECTS[0], p=p, q=q, lag_bounds=LAGB)
    x0, lo, hi = object_starts(OBJECTS[0], p, q, NT, SEED)
    got = bm._starts(NT, SEED)
    assert all(np.array_equal(g, w) for g, w in zip(got, (x0, lo, hi)))
    assert names(fake) == ["carma_ctx_create", "carma_ctx_set_prior", "carma_pt_run", "carma_pt_stats"]
    check_start_sampler(fake, H, TA, YA, p, q, SEED)
    fake.world.fun = lambda B: np.array([np.inf, 7.0])[:B]
    k = mark(fake)
    best = bm.get_mle(ntrials=NT, seed=SEED)
    assert names(fake, k) == ["carma_ctx_create", "carma_ctx_set_prior", "carma_pt_run", "carma_pt_stats", "carma_bands_create",
                              "carma_bands_mle_batched"]
    a = fake.args("carma_bands_mle_batched")
    check_bands(fake, a[0], OBJECTS[0], p, q)
    assert np.array_equal(rd(a[1], (NT, dx)), x0) and val(a[2]) == NT and np.array_equal(rd(a[3], (dx,)), lo) and np.array_equal(rd(a[4], (dx,)), hi)
    assert null(a[5]) and scalars(a, range(6, 12)) == [2000, 8, FTOL, 1e-5, 1e-6, int(p > 1)]
    check_fit(best, x0[1] + 1.0, 7.0, 1)
    fake.world.fun = lambda B: np.array([3.0, 7.0])[:B]
    every = bm.get_mle(ntrials=NT, seed=SEED, return_all=True)
    assert len(every) == NT
    for i, r in enumerate(every):
        check_fit(r, x0[i] + 1.0, [3.0, 7.0][i], i)
    # the profile: L x ntrials starts in one run, the lags held; a start without a finite value never wins
    lags = [-1.0, 0.5, 2.0]
    fake.world.fun = lambda B: np.array([5.0, 4.0, np.nan, 6.0, -np.inf, np.inf])[:B]
    k = mark(fake)
    ll, xs = bm.lag_profile(lags, ntrials=NT, seed=SEED)
    assert names(fake, k) == ["carma_ctx_create", "carma_ctx_set_prior", "carma_pt_run", "carma_pt_stats", "carma_bands_mle_batched"]
    a = fake.args("carma_bands_mle_batched")
    assert np.array_equal(rd(a[1], (3 * NT, dx)), np.tile(x0, (3, 1))) and val(a[2]) == 3 * NT
    assert np.array_equal(rd(a[3], (dx,)), lo) and np.array_equal(rd(a[4], (dx,)), hi)
    assert rd(a[5], (3 * NT, 1)).ravel().tolist() == [-1.0, -1.0, 0.5, 0.5, 2.0, 2.0] and val(a[11]) == int(p > 1)
    assert ll.tolist() == [-4.0, -6.0, -1e300] and np.array_equal(xs, np.stack([x0[1], x0[1], x0[0]]) + 1.0)
    with pytest.raises(ValueError, match="every lag must lie inside its box"):
        bm.lag_profile([0.0, 3.5])
    with pytest.raises(ValueError, match=r"lags must be \[L\] for two bands or \[L, 1\]"):
        bm.lag_profile(np.zeros((2, 2)))


def test_bandsmodel_smooth_and_smooth_band(fake):
    bm = cpa.CarmaBandsModel(OBJECTS[0], p=2, q=1, lag_bounds=LAGB)
    th = ramp((3, 9))
    mean, var = bm.smooth(th, [9.0, 8.0], band=1)
    assert names(fake) == ["carma_bands_create", "carma_bands_smooth"]
    a = fake.args("carma_bands_smooth")
    assert a[0] == H and np.array_equal(rd(a[1], (3, 9)), th) and scalars(a, (2, 3, 5)) == [3, 1, 2] and rd(a[4], (2,)).tolist() == [9.0, 8.0]
    assert null(a[8]) and null(a[9])
    assert np.array_equal(mean, ramp((3, 2), 10.0)) and np.array_equal(var, ramp((3, 2), 1.0))
    mean, var = bm.smooth(th[0], 4.5)                                            # one vector, one time, band 0
    a = fake.args("carma_bands_smooth")
    assert scalars(a, (2, 3, 5)) == [1, 0, 1] and mean.tolist() == [0.0] and var.tolist() == [1.0]
    bmean, bvar = bm.smooth_band(th, [9.0, 8.0], band=1)
    a = fake.args("carma_bands_smooth")
    assert scalars(a, (2, 3, 5)) == [3, 1, 2] and not null(a[8]) and bmean.tolist() == ramp((2,), 20.0).tolist() and bvar.tolist() == ramp((2,), 30.0).tolist()
    fake.world.invalid = [0, 0, 1]
    for call in (bm.smooth, bm.smooth_band):
        with pytest.raises(ValueError, match="CarmaBandsModel.smooth: row 2 has a repeated AR root"):
            call(th, [9.0, 8.0])


@pytest.mark.parametrize("p,q", [(1, 0), (2, 1)])
def test_bandsmodel_run_mcmc(fake, p, q):
    d = dim(p, q)
    dx = d + 3
    bm = cpa.CarmaBandsModel(OBJECTS[0], p=p, q=q, lag_bounds=LAGB)
    smp = bm.run_mcmc(NS, ntemperatures=NTEMP, nreplicas=NR, seed=SEED)          # the default box
    assert names(fake) == ["carma_bands_create", "carma_bands_pt_default_box", "carma_bands_pt_run", "carma_sigma_noise_batch",
                           "carma_bands_logdensity_batch"]
    check_bands(fake, H, OBJECTS[0], p, q)
    a = fake.args("carma_bands_pt_run")
    assert a[0] == H and scalars(a, range(1, 6)) == [NTEMP, NR, NS, NS // 2, 1] and null(a[6]) and val(a[7]) == SEED
    assert np.array_equal(rd(a[8], (1, 2)), ramp((1, 2), -7.0)) and np.array_equal(rd(a[9], (1, 2)), ramp((1, 2), 7.0))
    samples, logposts = ramp((NR, NS, dx), 0.1), ramp((NR, NS), -5.0)
    flat = samples.reshape(-1, dx)
    assert type(smp) is cpa.CarmaBandsSample and bm.mcmc_sample is smp and smp.model is bm
    assert np.array_equal(smp._all[0], samples) and np.array_equal(smp._all[1], logposts) and np.array_equal(smp.trace, flat)
    a = fake.args("carma_sigma_noise_batch")
    roots, ma, var = cpa.CarmaSample._sigma_inputs_of(flat[:, :d], p, q)
    assert scalars(a, (0, 1, 5)) == [p, q + 1, NR * NS] and np.array_equal(rd(a[2], (NR * NS, p, 2)), np.stack([roots.real, roots.imag], axis=-1))
    assert np.array_equal(rd(a[3], (NR * NS, q + 1)), ma) and np.array_equal(rd(a[4], (NR * NS,)), var)
    a = fake.args("carma_bands_logdensity_batch")
    assert np.array_equal(rd(a[1], (NR * NS, dx)), flat) and scalars(a, (2, 3)) == [NR * NS, 1]
    assert np.array_equal(smp._samples["sigma"][:, 0], ramp((NR * NS,), 0.5)) and np.array_equal(smp._samples["loglik"][:, 0], 100.0 + np.arange(NR * NS))
    assert np.array_equal(smp._samples["lag"][:, 0], flat[:, d]) and np.array_equal(smp._samples["logpost"][:, 0], logposts.ravel())
    # given boxes, an init, the other scalars
    init = ramp((dx,), 0.3)
    bm.run_mcmc(NS, nburnin=7, nthin=2, init=init, seed=SEED, scale_bounds=[(0.5, 4.0)], offset_bounds=[(-3.0, 9.0)])
    a = fake.args("carma_bands_pt_run")
    assert scalars(a, range(1, 6)) == [max(10, p + q), 1, NS, 7, 2] and np.array_equal(rd(a[6], (dx,)), init)
    assert rd(a[8], (1, 2)).tolist() == [[np.log(0.5), -3.0]] and rd(a[9], (1, 2)).tolist() == [[np.log(4.0), 9.0]]
    bm.run_mcmc(NS, seed=SEED, offset_bounds=[(-3.0, 9.0)])                      # one of the two: the other keeps its default
    a = fake.args("carma_bands_pt_run")
    assert rd(a[8], (1, 2)).tolist() == [[-7.0, -3.0]] and rd(a[9], (1, 2)).tolist() == [[7.0, 9.0]]
    for kw, msg in ((dict(nsamples=0), "nsamples"), (dict(nthin=0), "nthin"), (dict(nreplicas=0), "nreplicas"),
                    (dict(init=init[:3]), r"init must be \[%d\]" % dx), (dict(scale_bounds=[(0.0, 1.0)]), "scale_bounds: need 0 < lo <= hi"),
                    (dict(scale_bounds=[(1.0, 2.0)] * 2), "scale_bounds must hold one"), (dict(offset_bounds=[(2.0, 1.0)]), "offset_bounds: need lo <= hi")):
        k = mark(fake)
        with pytest.raises(ValueError, match=msg):
            bm.run_mcmc(**dict(dict(nsamples=NS), **kw))
        assert names(fake, k) == []
    # ntemperatures outside 1 ... 64 and a negative nburnin are refused here too, before a context exists
    fresh = cpa.CarmaBandsModel(OBJECTS[0], p=p, q=q, lag_bounds=LAGB)
    for kw, word in ((dict(ntemperatures=65), "ntemperatures"), (dict(ntemperatures=0), "ntemperatures"), (dict(nburnin=-1), "nburnin")):
        k = mark(fake)
        with pytest.raises(ValueError, match=word):
            fresh.run_mcmc(NS, **kw)
        assert names(fake, k) == [] and fresh._ctx is None


# ---- CarmaBandsSet --------------------------------------------------------------------------------------------
def check_bandset(fake, h, p, q):
    made = fake.world.made[h]
    assert made["kind"] == "bandset" and (made["p"], made["q"], made["S"], made["K"], made["off"]) == (p, q, 2, 2, [0, 4, 10, 16, 22])
    for i, key in enumerate("tye"):
        assert np.array_equal(made[key], np.concatenate([b[i] for o in OBJECTS for b in o]))
    assert made["lag"] == [[[-2.0], [-2.0]], [[3.0], [3.0]]] and made["ms"] == [pop_max_stdev(o[0][1]) for o in OBJECTS]


def test_bandsset_loglik_logpost(fake):
    bs = cpa.CarmaBandsSet(OBJECTS, p=2, q=1, lag_bounds=LAGB)
    th = ramp((3, 9))
    assert bs.loglik(th, [1, 0, 1]).tolist() == [100.0, 101.0, 102.0]
    assert names(fake) == ["carma_bandset_create", "carma_bandset_logdensity_batch"]
    check_bandset(fake, H, 2, 1)
    a = fake.args("carma_bandset_logdensity_batch")
    assert a[0] == H and np.array_equal(rd(a[1], (3, 9)), th) and rd(a[2], (3,), np.int32).tolist() == [1, 0, 1] and scalars(a, (3, 4)) == [3, 1]
    one = bs.logpost(th[1], 1)
    a = fake.args("carma_bandset_logdensity_batch")
    assert isinstance(one, float) and one == 100.0 and np.array_equal(rd(a[1], (1, 9)), th[1:2]) and scalars(a, (3, 4)) == [1, 0]
    assert rd(a[2], (1,), np.int32).tolist() == [1] and fake.count("carma_bandset_create") == 1
    with pytest.raises(ValueError, match="object index out of range"):
        bs.loglik(th, [0, 1, 2])


@pytest.mark.parametrize("p,q", [(1, 0), (2, 1)])
def test_bandsset_get_mle(fake, p, q):
    d = dim(p, q)
    dx = d + 3
    bs = cpa.CarmaBandsSet(OBJECTS, p=p, q=q, lag_bounds=LAGB)
    per = [object_starts(o, p, q, NT, SEED) for o in OBJECTS]
    lo, hi = np.stack([s[1] for s in per]), np.stack([s[2] for s in per])
    fake.world.fun = lambda B: np.array([3.0, 2.0, np.inf, 9.0])[:B]

    def check_call(want):
        a = fake.args("carma_bandset_mle_batched")
        check_bandset(fake, a[0], p, q)
        assert np.array_equal(rd(a[1], (2 * NT, dx)), want.reshape(2 * NT, dx)) and rd(a[2], (2 * NT,), np.int32).tolist() == [0, 0, 1, 1]
        assert val(a[3]) == 2 * NT and np.array_equal(rd(a[4], (2 * NT, dx)), lo[[0, 0, 1, 1]]) and np.array_equal(rd(a[5], (2 * NT, dx)), hi[[0, 0, 1, 1]])
        assert null(a[6]) and scalars(a, range(7, 13)) == [2000, 8, FTOL, 1e-5, 1e-6, int(p > 1)]

    fits = bs.get_mle(ntrials=NT, seed=SEED)                                     # None: each object's own starts
    assert names(fake) == ["carma_ctx_create", "carma_ctx_set_prior", "carma_pt_run", "carma_pt_stats"] * 2 + ["carma_bandset_create",
                                                                                                             "carma_bandset_mle_batched"]
    for s, o in enumerate(OBJECTS):
        check_start_sampler(fake, H + 8 * s, o[0][0], o[0][1], p, q, SEED)
    want = np.stack([s[0] for s in per])
    check_call(want)
    check_fit(fits[0], want[0, 1] + 1.0, 2.0, 1)
    check_fit(fits[1], want[1, 1] + 1.0, 9.0, 3)
    assert set(bs.timing) == {"starts_s", "optimise_s"}
    # "set": the CARMA part from one multi-series run over the objects' band 0 (both of 4 ... 6 data: longest first 1, 0)
    k = mark(fake)
    every = bs.get_mle(ntrials=NT, seed=SEED, starts="set", return_all=True)
    assert names(fake, k) == ["carma_mctx_create", "carma_mpt_run", "carma_bandset_mle_batched"]
    made = fake.world.made[fake.args("carma_mpt_run")[0]]
    assert made["kind"] == "mctx" and made["off"] == [0, 4, 10] and np.array_equal(made["y"], np.r_[YA, 2.0 * YB])
    assert made["ms"] == [pop_max_stdev(YA), pop_max_stdev(2.0 * YB)]
    a = fake.args("carma_mpt_run")
    assert rd(a[1], (2,), np.int32).tolist() == [1, 0] and scalars(a, range(2, 8)) == [2, 1 if p == 1 else 10, NT, 1, 25, 1] and val(a[9]) == SEED
    raw = ramp((2, NT, 1, d), 0.1)[:, :, 0, :]
    want = np.stack([ref_band_starts(o, ref_starts(raw[1 - s], ref_bounds(o[0][0], o[0][1], p, q), SEED), LAGB, SEED) for s, o in enumerate(OBJECTS)])
    check_call(want)
    for i in range(2 * NT):
        check_fit(every[i // NT][i % NT], want[i // NT, i % NT] + 1.0, [3.0, 2.0, np.inf, 9.0][i], i)
    k = mark(fake)
    given = ramp((2, NT, dx), 0.7)                                               # an array: nothing is drawn
    fits = bs.get_mle(starts=given)
    assert names(fake, k) == ["carma_bandset_mle_batched"]
    check_call(given)
    check_fit(fits[1], given[1, 1] + 1.0, 9.0, 3)
    for starts, msg in (("nope", "starts must be None, 'set' or an array"), (given[:, :, :d], r"starts must be \[2, ntrials, %d\]" % dx)):
        with pytest.raises(ValueError, match=msg):
            bs.get_mle(starts=starts)


def test_bandsset_lag_profile(fake):
    p, q, dx = 2, 1, 9
    bs = cpa.CarmaBandsSet(OBJECTS, p=p, q=q, lag_bounds=LAGB)
    per = [object_starts(o, p, q, NT, SEED) for o in OBJECTS]
    funs = np.array([5.0, 4.0, np.nan, 6.0, 1.0, 2.0, 8.0, 7.0, 3.0, np.inf])
    fake.world.fun = lambda B: funs[:B]
    out = bs.lag_profile([-1.0, 0.5], ntrials=NT, seed=SEED)                     # one grid for both objects
    assert names(fake) == ["carma_ctx_create", "carma_ctx_set_prior", "carma_pt_run", "carma_pt_stats"] * 2 + ["carma_bandset_create",
                                                                                                             "carma_bandset_mle_batched"]
    a = fake.args("carma_bandset_mle_batched")
    B = 2 * 2 * NT
    assert np.array_equal(rd(a[1], (B, dx)), np.concatenate([np.tile(s[0], (2, 1)) for s in per])) and rd(a[2], (B,), np.int32).tolist() == [0] * 4 + [1] * 4
    assert val(a[3]) == B and np.array_equal(rd(a[4], (B, dx)), np.repeat(np.stack([s[1] for s in per]), 4, axis=0))
    assert np.array_equal(rd(a[5], (B, dx)), np.repeat(np.stack([s[2] for s in per]), 4, axis=0))
    assert rd(a[6], (B, 1)).ravel().tolist() == [-1.0, -1.0, 0.5, 0.5] * 2 and val(a[12]) == 1
    assert [o[0].tolist() for o in out] == [[-4.0, -6.0], [-1.0, -7.0]]
    assert np.array_equal(out[0][1], per[0][0][[1, 1]] + 1.0) and np.array_equal(out[1][1], per[1][0][[0, 1]] + 1.0)
    k = mark(fake)
    out = bs.lag_profile([[-1.0, 0.5, 2.0], [0.0, 1.0]], ntrials=NT, seed=SEED)  # a grid per object: 3 and 2 lags
    assert names(fake, k) == ["carma_ctx_create", "carma_ctx_set_prior", "carma_pt_run", "carma_pt_stats"] * 2 + ["carma_bandset_mle_batched"]
    a = fake.args("carma_bandset_mle_batched")
    assert val(a[3]) == 10 and rd(a[2], (10,), np.int32).tolist() == [0] * 6 + [1] * 4
    assert rd(a[6], (10, 1)).ravel().tolist() == [-1.0, -1.0, 0.5, 0.5, 2.0, 2.0, 0.0, 0.0, 1.0, 1.0]
    assert np.array_equal(rd(a[1], (10, dx)), np.concatenate([np.tile(per[0][0], (3, 1)), np.tile(per[1][0], (2, 1))]))
    assert [o[0].tolist() for o in out] == [[-4.0, -6.0, -1.0], [-7.0, -3.0]]
    assert np.array_equal(out[0][1], per[0][0][[1, 1, 0]] + 1.0) and np.array_equal(out[1][1], per[1][0][[1, 0]] + 1.0)
    assert set(bs.timing) == {"starts_s", "optimise_s"}
    with pytest.raises(ValueError, match="object 1: every lag must lie inside its box"):
        bs.lag_profile([[0.0], [3.5]])
    with pytest.raises(ValueError, match=r"lags must be \[L\] for two bands or \[L, 1\], for all objects or a list of one per object"):
        bs.lag_profile(np.zeros((2, 2)))


def test_bandsset_smooth(fake):
    bs = cpa.CarmaBandsSet(OBJECTS, p=2, q=1, lag_bounds=LAGB)
    v0, rows1 = ramp((9,), 0.2), ramp((2, 9), 0.4)                               # object 0: one vector; object 1: two rows
    out = bs.smooth([v0, rows1], [9.0, 8.0])                                     # band None: both bands
    assert names(fake) == ["carma_bandset_create", "carma_bandset_smooth"]
    check_bandset(fake, H, 2, 1)
    a = fake.args("carma_bandset_smooth")
    assert a[0] == H and val(a[4]) == 6 and np.array_equal(rd(a[1], (6, 9)), np.concatenate([v0[None], v0[None], rows1, rows1]))
    assert rd(a[2], (6,), np.int32).tolist() == [0, 0, 1, 1, 1, 1] and rd(a[3], (6,), np.int32).tolist() == [0, 1, 0, 0, 1, 1]
    assert rd(a[5], (12,)).tolist() == [9.0, 8.0] * 6 and rd(a[6], (7,), np.int64).tolist() == [0, 2, 4, 6, 8, 10, 12]
    m, v = ramp((12,)), ramp((12,), 1.0)
    assert out[0][0].shape == (2, 2) and np.array_equal(out[0][0], m[:4].reshape(2, 2)) and np.array_equal(out[0][1], v[:4].reshape(2, 2))
    assert out[1][0].shape == (2, 2, 2) and np.array_equal(out[1][0], m[4:].reshape(2, 2, 2)) and np.array_equal(out[1][1], v[4:].reshape(2, 2, 2))

    class Fit:
        def __init__(self, x):
            self.x = x
    out = bs.smooth([Fit(v0), rows1], [[9.0, 8.0, 7.0], [6.0]], band=1)          # an int: no band axis; times per object; a fit's .x
    a = fake.args("carma_bandset_smooth")
    assert val(a[4]) == 3 and rd(a[2], (3,), np.int32).tolist() == [0, 1, 1] and rd(a[3], (3,), np.int32).tolist() == [1, 1, 1]
    assert rd(a[5], (5,)).tolist() == [9.0, 8.0, 7.0, 6.0, 6.0] and rd(a[6], (4,), np.int64).tolist() == [0, 3, 4, 5]
    assert out[0][0].tolist() == [0.0, 0.01, 0.02] and out[1][0].tolist() == [[0.03], [0.04]] and out[1][1].tolist() == [[1.03], [1.04]]
    out = bs.smooth([rows1, v0], 4.5, band=[1, 0])                               # a list: the bands in the caller's order
    a = fake.args("carma_bandset_smooth")
    assert rd(a[2], (6,), np.int32).tolist() == [0, 0, 0, 0, 1, 1] and rd(a[3], (6,), np.int32).tolist() == [1, 1, 0, 0, 1, 0]
    assert out[0][0].shape == (2, 2, 1) and out[1][0].shape == (2, 1) and out[1][0].tolist() == [[0.04], [0.05]]
    out = bs.smooth([v0, rows1], np.array([[9.0, 8.0], [7.0, 6.0]]), band=0)    # an array [S, M]: a row of times per object
    a = fake.args("carma_bandset_smooth")
    assert rd(a[5], (6,)).tolist() == [9.0, 8.0, 7.0, 6.0, 7.0, 6.0] and rd(a[6], (4,), np.int64).tolist() == [0, 2, 4, 6]
    assert out[0][0].shape == (2,) and out[1][0].shape == (2, 2)
    k = mark(fake)
    with pytest.raises(ValueError, match=r"time must be one array, or one per object \(2\), got 3"):
        bs.smooth([v0, rows1], [[9.0], [8.0], [7.0]])
    assert names(fake, k) == []
    # an invalid row is named by its object and its row among that object's
    fake.world.invalid = [0, 0, 0, 0, 0, 1]
    with pytest.raises(ValueError, match="CarmaBandsSet.smooth: object 1, row 1 has a repeated AR root"):
        bs.smooth([v0, rows1], [9.0, 8.0])
    fake.world.invalid = [0, 1, 0, 0, 0, 0]
    with pytest.raises(ValueError, match="CarmaBandsSet.smooth: object 0, row 0 has"):
        bs.smooth([v0, rows1], [9.0, 8.0])
    with pytest.raises(ValueError, match=r"thetas must hold one entry per object \(2\), got 1"):
        bs.smooth([v0], [9.0])
    with pytest.raises(ValueError, match=r"object 1: thetas must be \[9\] or \[B, 9\]"):
        bs.smooth([v0, rows1[:, :5]], [9.0])


def test_bandsset_run_mcmc(fake):
    p, q, d, dx, M = 2, 1, 6, 9, 3
    bs = cpa.CarmaBandsSet(OBJECTS, p=p, q=q, lag_bounds=LAGB)
    which = [0, 1, 0]                                                            # 10, 12, 10 data: longest first is entry 1, then 0, 2
    init = ramp((M, dx), 0.3)
    sb = np.array([[(0.5, 4.0)], [(0.25, 8.0)], [(0.125, 16.0)]])                # a box per entry of which
    out = bs.run_mcmc(NS, ntemperatures=NTEMP, nreplicas=NR, seed=SEED, which=which, init=init, scale_bounds=sb, offset_bounds=[(-3.0, 9.0)])
    assert names(fake) == ["carma_bandset_create"] + ["carma_bandset_pt_default_box"] * 3 + ["carma_bandset_pt_run", "carma_bandset_logdensity_batch",
                                                                                          "carma_sigma_noise_batch"]
    check_bandset(fake, H, p, q)
    assert [val(fake.args("carma_bandset_pt_default_box", k)[1]) for k in range(3)] == which
    a = fake.args("carma_bandset_pt_run")
    assert a[0] == H and rd(a[1], (M,), np.int32).tolist() == [1, 0, 0] and scalars(a, range(2, 8)) == [M, NTEMP, NR, NS, NS // 2, 1]
    assert np.array_equal(rd(a[8], (M, dx)), init[[1, 0, 2]]) and val(a[9]) == SEED
    assert rd(a[10], (M, 1, 2)).tolist() == [[[np.log(0.25), -3.0]], [[np.log(0.5), -3.0]], [[np.log(0.125), -3.0]]]
    assert rd(a[11], (M, 1, 2)).tolist() == [[[np.log(8.0), 9.0]], [[np.log(4.0), 9.0]], [[np.log(16.0), 9.0]]]
    samples, logposts = ramp((M, NR, NS, dx), 0.1), ramp((M, NR, NS), -5.0)
    flat, per = samples.reshape(-1, dx), NR * NS
    a = fake.args("carma_bandset_logdensity_batch")
    assert np.array_equal(rd(a[1], (M * per, dx)), flat) and rd(a[2], (M * per,), np.int32).tolist() == [1] * per + [0] * 2 * per
    assert scalars(a, (3, 4)) == [M * per, 1]
    a = fake.args("carma_sigma_noise_batch")
    roots, ma, var = cpa.CarmaSample._sigma_inputs_of(flat[:, :d], p, q)
    assert scalars(a, (0, 1, 5)) == [p, q + 1, M * per] and np.array_equal(rd(a[2], (M * per, p, 2)), np.stack([roots.real, roots.imag], axis=-1))
    assert np.array_equal(rd(a[3], (M * per, q + 1)), ma) and np.array_equal(rd(a[4], (M * per,)), var)
    assert len(out) == M
    for j, i in enumerate((1, 0, 2)):                                            # run j is entry i of which
        smp = out[i]
        assert type(smp) is cpa.CarmaBandsSample and smp.model is bs.models[which[i]]
        assert np.array_equal(smp._all[0], samples[j]) and np.array_equal(smp._all[1], logposts[j])
        assert np.array_equal(smp._samples["loglik"][:, 0], 100.0 + per * j + np.arange(per))
        assert np.array_equal(smp._samples["sigma"][:, 0], ramp((M * per,), 0.5)[per * j:per * (j + 1)])
    assert bs.models[0].mcmc_sample is out[2] and bs.models[1].mcmc_sample is out[1]
    # the defaults: every object, its default box, no init
    k = mark(fake)
    out = bs.run_mcmc(NS, seed=SEED)
    assert names(fake, k) == ["carma_bandset_pt_default_box"] * 2 + ["carma_bandset_pt_run", "carma_bandset_logdensity_batch", "carma_sigma_noise_batch"]
    a = fake.args("carma_bandset_pt_run")
    assert rd(a[1], (2,), np.int32).tolist() == [1, 0] and scalars(a, range(2, 8)) == [2, 10, 1, NS, NS // 2, 1] and null(a[8])
    assert np.array_equal(rd(a[10], (2, 1, 2)), np.stack([ramp((1, 2), -8.0), ramp((1, 2), -7.0)]))
    assert np.array_equal(rd(a[11], (2, 1, 2)), np.stack([ramp((1, 2), 8.0), ramp((1, 2), 7.0)]))
    assert np.array_equal(out[0]._all[0], ramp((2, 1, NS, dx), 0.1)[1]) and np.array_equal(out[1]._all[0], ramp((2, 1, NS, dx), 0.1)[0])
    bs.run_mcmc(NS, seed=SEED, init=init[0], which=[1])                          # one vector for every run
    a = fake.args("carma_bandset_pt_run")
    assert rd(a[1], (1,), np.int32).tolist() == [1] and np.array_equal(rd(a[8], (1, dx)), init[:1])
    for kw, msg in ((dict(nsamples=0), "nsamples"), (dict(nthin=0), "nthin"), (dict(nreplicas=0), "nreplicas"),
                    (dict(ntemperatures=65), "ntemperatures"), (dict(nburnin=-1), "nburnin"), (dict(which=[]), "which"),
                    (dict(which=[2]), "which"), (dict(init=init, which=[0, 1]), r"init must be \[9\] or \[2, 9\]"),
                    (dict(scale_bounds=sb), r"scale_bounds must be \[1, 2\] for all objects or \[2, 1, 2\]"),
                    (dict(scale_bounds=[[(1.0, 2.0)], [(0.0, 1.0)]]), "object 1: scale_bounds: need 0 < lo <= hi"),
                    (dict(offset_bounds=[(2.0, 1.0)]), "object 0: offset_bounds: need lo <= hi")):
        k = mark(fake)
        with pytest.raises(ValueError, match=msg):
            bs.run_mcmc(**dict(dict(nsamples=NS), **kw))
        assert names(fake, k) == []
