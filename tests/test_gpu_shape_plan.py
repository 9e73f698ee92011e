"""The library's answers on a device against the restatement tests/shape_plan_ref.py (tests/test_shape_plan_cpu.py holds the
header carma_shape_plan.h to the same restatement): Context.kernel_name over the evaluation counts at which the log-density launch
changes kernels, and the sampler's family and row pipeline over the ladder counts at which the sampler changes, all scaled to the
device's own CU count (read through torch).  Only three samplers launch anything (n = 40, T = 4, two iterations)."""
import os

import numpy as np
import pytest

import shape_plan_ref as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RING3L = 43584            # Pipe3LGeom<2>::BYTES (tests/test_shape_plan_cpu.py)
ROW_PER_CU = 3            # k_pt_row<P,3>: 168 registers, three workgroups per CU


@pytest.fixture(scope="module")
def cpa():
    import carma_pack_amd
    assert carma_pack_amd._lib.lib.carma_device_count() >= 1, "no MI355X visible"
    return carma_pack_amd


@pytest.fixture(scope="module")
def cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def readme():
    g = np.load(os.path.join(HERE, "golden", "carma53_readme.npz"))
    return g["t"], g["y"], g["yerr"]


def env_switches():
    """the switches the library read from the environment when it was loaded"""
    return ref.switches(**{k: int(os.environ["CARMA_TUNE_" + k.upper()]) for k in ref.SW_NAMES
                           if k not in ("pt_row_rot", "pt_plain") and os.environ.get("CARMA_TUNE_" + k.upper()) is not None})


@pytest.mark.parametrize("p", [2, 3, 4, 5, 6, 7])
def test_kernel_names(cpa, cus, readme, p):
    """the evaluation counts of tests/test_shape_plan_cpu.py's literal cases that do not depend on the lpc kernel's occupancy -- up to
    one lpc workgroup per CU, and from three on -- times #CUs / 256, each - 1, itself and + 1; the README series, one that suits no
    window pipeline (a close pair of data), a regular cadence, 15 data"""
    t, y, e = readme
    k = 100
    reg = np.arange(90.0) * 0.75
    series = [(t, y, e), (np.insert(t, k + 1, t[k] + 0.01), np.insert(y, k + 1, y[k]), np.insert(e, k + 1, e[k])), (reg, y[:90], e[:90]),
              (t[:15], y[:15], e[:15])]
    counts = sorted({b for f in (2, 4, 6, 12, 16, 32, 64, 192, 193, 256) for b in (f * cus - 1, f * cus, f * cus + 1)} | {1, 2048, 4096, 8192, 16384})
    counts = [b for b in counts if b <= 64 * cus or b > 192 * cus]
    for ts, ys, es in series:
        ctx = cpa.Context(ts, ys, es, p, p - 1)
        flags = ref.series_flags(np.sort(ts), p, ctx.prior()[1])
        for B in counts:
            assert ctx.kernel_name(B) == ref.kernel_name(p, B, len(ts), flags, cus, sw=env_switches()), (p, B, len(ts), flags)


def test_car1_kernel_name(cpa, readme):
    t, y, e = readme
    ctx = cpa.Context(t, y, e, 1, 0)
    assert ctx.kernel_name(1) == ctx.kernel_name(10 ** 5) == "k_logdens_car1"


def test_sampler_family(cpa, cus, readme, monkeypatch):
    """T = 16, p = 5 on the README series: the ladder counts 64, 65, 129, 192, 193, 256, 257 of 256 CUs, on this device's; the forced
    kernels; T = 65, where the lane kernel is refused; CAR(1) around its thresholds, with 63 and 64 data.  Nothing is launched."""
    t, y, e = readme
    n, sw = len(t), env_switches()
    monkeypatch.delenv("CARMA_TUNE_PT_LANE_MIN", raising=False)
    ctx = cpa.Context(t, y, e, 5, 3)
    for R in (cus // 4, cus // 4 + 1, cus // 2 + 1, 3 * cus // 4, 3 * cus // 4 + 1, cus, cus + 1):
        for force in (None, "ladder", "row", "lane"):
            if force is None:
                monkeypatch.delenv("CARMA_PT_KERNEL", raising=False)
            else:
                monkeypatch.setenv("CARMA_PT_KERNEL", force)
            ctx.pt_create(16, R, adapt_iters=10)
            assert ctx.pt_kernel() == ("ladder", "row", "lane")[ref.family(5, 16, R, n, cus, ROW_PER_CU, force, sw=sw)], (R, force)
    monkeypatch.setenv("CARMA_PT_KERNEL", "lane")
    ctx.pt_create(65, 1, adapt_iters=10)
    assert ctx.pt_kernel() == "row" == ("ladder", "row", "lane")[ref.family(5, 65, 1, n, cus, ROW_PER_CU, "lane", sw=sw)]
    monkeypatch.delenv("CARMA_PT_KERNEL", raising=False)
    monkeypatch.setenv("CARMA_TUNE_PT_LANE_MIN", str(16 * 8))
    ctx.pt_create(16, 8, adapt_iters=10)
    assert ctx.pt_kernel() == "lane"
    monkeypatch.delenv("CARMA_TUNE_PT_LANE_MIN", raising=False)
    for m in (63, 64):
        c1 = cpa.Context(t[:m], y[:m], e[:m], 1, 0)
        for nchain in (63, 64, 48 * cus, 48 * cus + 1, 64 * cus, 64 * cus + 1):
            c1.pt_create(1, nchain, adapt_iters=10)
            assert c1.pt_kernel() == ("ladder", "row", "lane")[ref.family(1, 1, nchain, m, cus, 0)], (m, nchain)


@pytest.mark.parametrize("which", ["two ladders", "half the CUs and one", "every CU and one"])
def test_row_pipeline(cpa, cus, which, monkeypatch):
    """n = 40, T = 4, p = 5: R = 2 (two-sided, a CU per workgroup), #CUs / 2 + 1 (two-sided, workgroups share CUs) and #CUs + 1 (more
    than two workgroups per CU in the two-sided form: the one-datum pipeline, a ladder per workgroup); two iterations each"""
    from carma_pack_amd.synth import irregular_series
    R = {"two ladders": 2, "half the CUs and one": cus // 2 + 1, "every CU and one": cus + 1}[which]
    t, y, e = irregular_series(40, seed=5)
    ctx = cpa.Context(t, y, e, 5, 3)
    flags = ref.series_flags(t, 5, ctx.prior()[1])
    monkeypatch.delenv("CARMA_PT_KERNEL", raising=False)
    monkeypatch.delenv("CARMA_TUNE_PT_LANE_MIN", raising=False)
    ctx.pt_create(4, R, adapt_iters=10, seed=3)
    assert ctx.pt_kernel() == "row" == ("ladder", "row", "lane")[ref.family(5, 4, R, 40, cus, ROW_PER_CU, sw=env_switches())]
    ctx.pt_start(None)
    ctx.pt_iterate(2)
    assert ctx.pt_kernel() == "row"                           # (the launch was taken: no fall-back to the ladder kernel)
    pl = ref.row(R, 4, 4, 40, flags, cus, ref.row_lds(RING3L, 4, 40), env_switches())
    assert cpa.Context.pt_row_pipeline() == ref.PIPELINES[pl["pipeline"]], (R, flags, pl)
    assert np.all(np.isfinite(ctx.pt_get_chains()[1]))
